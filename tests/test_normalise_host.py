"""Normalising the observed set without a device: the refusals and their order, the extents, the tiles and the arithmetic of
transit_amd/csrc/trx_normalise.h through tests/normalise_check.cpp, a stand-alone program over exact-size heap arrays under
-fsanitize=address,undefined that walks a whole set the way the kernels do -- one block's lanes per row, the same bisection
and staging capacity, one lane per column --; its data, row scales, centres and counts held bit for bit against
xcor.normalise_reference, the numpy mirror, whose quantile comes from a full sort; the rank formula; a noise-free set whose
normalised data are zero to a few roundings; planted outliers under the clip; the mirror's own properties; and the ABI: the
struct's size, the constants, the exported symbols and the kernels in the code object."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from bits import same_bits
from host_check import build_check

import many_cases as mc
import normalise_cases as nc
import sysrem_cases as sc
from transit_amd import _abi, build, xcor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("normalise_check", tmp_path_factory.mktemp("normalise_check"))


def test_refusals_in_order_extents_tiles_bisection_and_known_sets_under_sanitizers(check_exe):
    out = subprocess.run([check_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == ""                              # (no sanitizer report)
    lines = out.stdout.splitlines()
    last = lines[-1].split()
    assert last[0] == "ok" and int(last[1]) > 300, lines[-20:]
    assert not [line for line in lines if line.startswith("FAILED")]


def program(check_exe, path, data, w, seg, nm):
    """the program's (data, scale, centre, nclipped, nbad) of one set under one recipe"""
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %s %s\n%s\n" % (data.shape[0], len(seg) - 1, int(w is not None), nm.row_kind, nm.col_kind, float(nm.quantile).hex(),
                                              float(nm.clip).hex(), " ".join(str(int(x)) for x in seg)))
        for arr in (data,) + ((w,) if w is not None else ()):
            f.write(" ".join(float(x).hex() for x in arr.reshape(-1)) + "\n")
    out = subprocess.run([check_exe, "set", str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-4000:]
    lines = {w_[0]: w_[1:] for w_ in (line.split() for line in out.stdout.splitlines())}
    assert "FAILED" not in lines
    got = {k: np.array([float.fromhex(x) for x in lines[k]]) for k in ("data", "scale", "centre")}
    return got["data"].reshape(data.shape), got["scale"].reshape(data.shape[0], len(seg) - 1), got["centre"], int(lines["nclipped"][0]), int(lines["nbad"][0])


def sets(which):
    if which == "sysrem set, edge weights":
        return sc.data_set(7, 77), sc.edge_weights(7, 87), sc.SEG
    if which == "sysrem set, no weights":
        return sc.data_set(12, 82), None, sc.SEG
    if which == "edge set, weights":
        return nc.the_set(7, True) + (nc.SEG,)
    return nc.the_set(2, False) + (nc.SEG,)


@pytest.mark.parametrize("which", ["sysrem set, edge weights", "sysrem set, no weights", "edge set, weights", "edge set, no weights"])
def test_the_programs_outputs_are_the_mirrors_bit_for_bit(check_exe, tmp_path, which):
    data, w, seg = sets(which)
    recipes = nc.recipes() if "weights" in which and "no weights" not in which else nc.recipes()[::5]
    for nm in recipes:
        want = xcor.normalise_reference(data, w, seg, nm)
        got = program(check_exe, tmp_path / "set.txt", data, w, seg, nm)
        what = which + ", " + nc.name(nm)
        for g, m in zip(got[:3], want[:3]):
            assert same_bits(g, m), what
        assert got[3:] == want[3:], what
        out, scale, centre, nclipped, nbad = want
        assert np.isfinite(out).all() and not np.signbit(scale).any() and np.all(scale >= 0), what
        live = np.ones_like(data, dtype=bool) if w is None else w > 0
        assert np.all(out[~live] == 0) and not np.signbit(out[~live]).any(), what
        if nm.row_kind == xcor.NORM_ROW_NONE:
            assert np.all((scale == 1.0) | (scale == 0.0)), what
        if nm.clip == 0:
            assert nclipped == 0, what


LONG_RECIPES = [xcor.Normalise(xcor.NORM_ROW_QUANTILE, xcor.NORM_COL_RATIO, 0.5, 0.0), xcor.Normalise(xcor.NORM_ROW_QUANTILE, xcor.NORM_COL_DIVIDE, 0.9, 3.0)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nm", LONG_RECIPES, ids=nc.name)
def test_the_programs_outputs_on_the_long_orders(check_exe, tmp_path, nm, weighted):
    """many_cases.long_set under the two recipes of tests/test_gpu_long_orders.py: rows of 1024 and 1025 keys below the staging
    capacity, of 2049 one above it; the quantile against a full sort, and the mirror's median against np.sort's lower middle"""
    ms = mc.long_set()[0]
    w = ms.weight if weighted else None
    want = xcor.normalise_reference(ms.data, w, ms.seg_first, nm)
    got = program(check_exe, tmp_path / "set.txt", ms.data, w, ms.seg_first, nm)
    for g, m in zip(got[:3], want[:3]):
        assert same_bits(g, m), nc.name(nm)
    assert got[3:] == want[3:], nc.name(nm)
    out, scale, centre, nclipped, nbad = want
    live = np.ones_like(ms.data, dtype=bool) if w is None else w > 0
    assert np.isfinite(out).all() and np.all(out[~live] == 0) and not np.signbit(out[~live]).any()
    assert np.all(scale[:, 2] == 0) and np.all(scale[:, [0, 3, 4]] > 0) and (nm.clip > 0 or nclipped == 0)
    assert (scale[ms.masked_exp, ms.masked_seg] == 0) == weighted and np.count_nonzero(scale[:, ms.masked_seg] > 0) == ms.nexp - int(weighted)
    for v in range(ms.nexp):
        for s in range(ms.nseg):
            x = ms.data[v, ms.segment(s)][live[v, ms.segment(s)]]
            if x.size == 0:
                assert scale[v, s] == 0
                continue
            k = int(np.floor(nm.quantile * (x.size - 1)))
            assert scale[v, s] == np.sort(x)[k] and (nm.quantile != 0.5 or k == (x.size - 1) // 2)


def test_the_edge_set_has_its_edges():
    """what normalise_cases promises: ties, an all-equal row, negative values, a masked row, rows of a quantile <= 0, and the
    two segments about the staging capacity"""
    data, w = nc.the_set(7, True)
    assert nc.LENGTHS[nc.OVER_SEG] == nc.CAP + 1 and nc.LENGTHS[nc.AT_SEG] == nc.CAP
    a, b = int(nc.SEG[nc.OVER_SEG]), int(nc.SEG[nc.OVER_SEG + 1])
    assert np.unique(data[0, a:b]).size < 20 and np.all(data[0, a:b] == np.round(data[0, a:b]))
    a, b = int(nc.SEG[nc.ODD_SEG]), int(nc.SEG[nc.ODD_SEG + 1])
    assert np.unique(data[0, a:b]).size == 1 and np.all(data[1, a:b] < 0)
    a, b = int(nc.SEG[nc.TIE_SEG]), int(nc.SEG[nc.TIE_SEG + 1])
    assert np.any(data[:, a:b] < 0) and np.any(data[:, a:b] == 0)
    assert np.all(w[6, nc.SEG[nc.MASKED_SEG]:nc.SEG[nc.MASKED_SEG + 1]] == 0)
    out, scale, centre, _, nbad = xcor.normalise_reference(data, w, nc.SEG, xcor.Normalise(xcor.NORM_ROW_QUANTILE, xcor.NORM_COL_RATIO, 0.5, 0.0))
    assert scale[6, nc.MASKED_SEG] == 0 and scale[1, nc.ODD_SEG] == 0 and scale[0, nc.ODD_SEG] == 2.5
    assert np.count_nonzero(scale[:, nc.TIE_SEG] == 0) >= 1 and nbad > 0           # (rows whose median is <= 0: bad)
    out0 = xcor.normalise_reference(data, w, nc.SEG, xcor.Normalise(xcor.NORM_ROW_QUANTILE, xcor.NORM_COL_RATIO, 0.0, 0.0))[1]
    assert np.all(out0[:, nc.TIE_SEG] == 0)                                        # (every row's minimum is <= 0 there)


@pytest.mark.parametrize("m", [1, 2, 3, 64, 65])
@pytest.mark.parametrize("q", [0.0, 0.5, 1.0, 0.9])
def test_the_rank_formula(check_exe, q, m):
    want = {0.0: 0, 0.5: (m - 1) // 2, 1.0: m - 1, 0.9: {1: 0, 2: 0, 3: 1, 64: 56, 65: 57}[m]}[q]
    out = subprocess.run([check_exe, "rank", float(q).hex(), str(m)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "" and int(out.stdout) == want
    assert int(math.floor(q * float(m - 1))) == want
    # the mirror takes the entry of that rank of the sorted live values: m distinct values, half of them masked away
    x = np.arange(2 * m, dtype=np.float64)[None, ::-1] + 1.0
    w = np.tile([1.0, 0.0], m)[None, :]
    scale = xcor.normalise_reference(x, w, [0, 2 * m], xcor.Normalise(xcor.NORM_ROW_QUANTILE, xcor.NORM_COL_NONE, q, 0.0))[1]
    assert scale[0, 0] == np.sort(x[0, w[0] > 0])[want]


def test_a_noise_free_set_is_flat_to_a_few_roundings(check_exe, tmp_path):
    """f0 = cont[p] * thr[v] without noise under QUANTILE 0.5 + RATIO: every row's median is thr[v] times the continuum's,
    every column's mean of f0 / scale is cont[p] over that, the ratio is 1: |data| <= 1e-14 -- a few roundings of values
    about 1: the product, the division by the scale, the mean, the ratio."""
    nexp, seg = 9, xcor.segments([70, 130])
    x = np.linspace(0.0, 1.0, 200)
    cont, thr = 1000.0 * (1.0 + 0.4 * np.sin(11.0 * x)), np.linspace(0.6, 1.3, nexp)
    f0 = cont[None, :] * thr[:, None]
    nm = xcor.Normalise(xcor.NORM_ROW_QUANTILE, xcor.NORM_COL_RATIO, 0.5, 0.0)
    for got in (xcor.normalise_reference(f0, None, seg, nm), program(check_exe, tmp_path / "flat.txt", f0, None, seg, nm)):
        data, scale, centre, nclipped, nbad = got
        print("largest |data| %.3e" % np.abs(data).max())
        assert np.abs(data).max() <= 1e-14 and nclipped == 0 and nbad == 0
        for s in range(2):
            med = np.sort(cont[seg[s]:seg[s + 1]])[(seg[s + 1] - seg[s] - 1) // 2]
            assert np.allclose(scale[:, s], thr * med, rtol=1e-15, atol=0)
            assert np.allclose(centre[seg[s]:seg[s + 1]], cont[seg[s]:seg[s + 1]] / med, rtol=1e-14, atol=0)


def test_planted_outliers_are_the_only_entries_the_clip_replaces(check_exe, tmp_path):
    """200 exposures x 64 pixels of a flat continuum with 1 % Gaussian noise (seed 4), clip = 8: the mirror clips nothing of
    the noise alone -- checked here --, and with one entry of 50 sigma planted in each of five columns exactly those five are
    replaced, by their column's mean."""
    nexp, npix, sigma = 200, 64, 0.01
    seg = [0, npix]
    f0 = 1.0 + sigma * np.random.default_rng(4).standard_normal((nexp, npix))
    clip8 = xcor.Normalise(xcor.NORM_ROW_QUANTILE, xcor.NORM_COL_RATIO, 0.5, 8.0)
    noclip = xcor.Normalise(xcor.NORM_ROW_QUANTILE, xcor.NORM_COL_RATIO, 0.5, 0.0)
    assert xcor.normalise_reference(f0, None, seg, clip8)[3] == 0                  # (the seed's precondition)
    planted = [(17, 3), (0, 20), (199, 21), (88, 40), (120, 63)]
    for v, p in planted:
        f0[v, p] += 50.0 * sigma
    want = xcor.normalise_reference(f0, None, seg, clip8)
    plain = xcor.normalise_reference(f0, None, seg, noclip)
    got = program(check_exe, tmp_path / "clip.txt", f0, None, seg, clip8)
    for out in (want, got):
        data, scale, centre, nclipped, nbad = out
        assert nclipped == len(planted) and nbad == 0
        differ = np.argwhere(data != plain[0])
        assert sorted(map(tuple, differ)) == sorted(planted)
        for v, p in planted:
            col = plain[0][:, p]
            s = 0.0
            for x in col:
                s = s + x
            assert data[v, p] == s / nexp and abs(data[v, p]) < 1e-2 and plain[0][v, p] > 0.4
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and same_bits(got[2], want[2])


def test_weights_none_are_weights_one_and_the_median_is_the_sorted_lower_middle():
    data = sc.data_set(7, 77)
    for nm in nc.recipes()[::4]:
        a, b = xcor.normalise_reference(data, None, sc.SEG, nm), xcor.normalise_reference(data, np.ones_like(data), sc.SEG, nm)
        assert all(same_bits(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]
    w = sc.edge_weights(7, 87)
    scale = xcor.normalise_reference(data, w, sc.SEG, xcor.Normalise(xcor.NORM_ROW_QUANTILE, xcor.NORM_COL_NONE, 0.5, 0.0))[1]
    for v in range(7):
        for s in range(len(sc.LENGTHS)):
            x = data[v, sc.SEG[s]:sc.SEG[s + 1]][w[v, sc.SEG[s]:sc.SEG[s + 1]] > 0]
            assert scale[v, s] == (np.sort(x)[(x.size - 1) // 2] if x.size else 0.0)
            if x.size % 2:
                assert scale[v, s] == np.median(x)
    assert scale[sc.MASKED_EXP, sc.MASKED_SEG] == 0 and np.all(scale[:, 5] == 0)    # the masked row, the empty segment


def test_the_mirror_refuses_what_it_does_not_define():
    for bad in (xcor.Normalise(2, 0), xcor.Normalise(1, 4), xcor.Normalise(1, 1, 1.5), xcor.Normalise(1, 1, 0.5, 0.5), xcor.Normalise(1, 1, float("nan"))):
        with pytest.raises(ValueError):
            xcor.normalise_reference(np.ones((3, 5)), None, [0, 5], bad)
    with pytest.raises(ValueError):
        xcor.normalise_reference(np.ones(5), None, [0, 5], xcor.Normalise(1, 1))


def test_abi_struct_constants_symbols_and_kernels():
    assert ctypes.sizeof(_abi.TrxNormalise) == 24
    assert (_abi.NORM_ROW_NONE, _abi.NORM_ROW_QUANTILE) == (0, 1) == (xcor.NORM_ROW_NONE, xcor.NORM_ROW_QUANTILE)
    assert (_abi.NORM_COL_NONE, _abi.NORM_COL_DIVIDE, _abi.NORM_COL_RATIO, _abi.NORM_COL_SUBTRACT) == (0, 1, 2, 3)
    assert (xcor.NORM_COL_NONE, xcor.NORM_COL_DIVIDE, xcor.NORM_COL_RATIO, xcor.NORM_COL_SUBTRACT) == (0, 1, 2, 3)
    c = xcor.Normalise(xcor.NORM_ROW_QUANTILE, xcor.NORM_COL_RATIO, 0.9, 5.0).to_c()
    assert (c.row_kind, c.col_kind, c.quantile, c.clip) == (1, 2, 0.9, 5.0)
    txt = open(os.path.join(ROOT, "include", "transit_hip.h")).read()
    for line in ("#define TRX_NORM_ROW_NONE      0", "#define TRX_NORM_ROW_QUANTILE  1", "#define TRX_NORM_COL_NONE      0", "#define TRX_NORM_COL_DIVIDE    1",
                 "#define TRX_NORM_COL_RATIO     2", "#define TRX_NORM_COL_SUBTRACT  3", "#define TRX_ABI_VERSION 5"):
        assert line in txt
    path = build.lib_path("libtransit_hip.so")
    if not os.path.exists(path):
        build.build_hip()
    lib = ctypes.CDLL(path)
    assert hasattr(lib, "trx_set_normalise") and hasattr(lib, "trx_normalise_observed")
    lib.trx_abi_version.restype = ctypes.c_int
    assert lib.trx_abi_version() == 5
    blob = open(path, "rb").read()
    for k in (b"k_norm_rowscale", b"k_norm_cols"):
        assert k in blob, k
    # refused without a handle, before anything is touched
    _abi.bind(lib, _abi.HIP_HEADER, "trx_")
    assert lib.trx_set_normalise(None, None) == -1
    assert lib.trx_normalise_observed(None, None, None, None, 0, None, 0, 0.0, 0.0, None, None, None, None, None, None) == -1
