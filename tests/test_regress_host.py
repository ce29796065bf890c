"""Regressing the observed set on given time vectors without a device: the refusals and their order, the extents and the
merge of transit_amd/csrc/trx_regress.h through tests/regress_check.cpp, a stand-alone program over exact-size heap arrays
under -fsanitize=address,undefined that walks a whole set the way k_wfilter_factor and k_regress_cols do -- one lane per
column, the factor component-major, the data in place --; its coefficients, residuals and singular count held bit for bit
against xcor.regress_reference, the numpy mirror; the bits' independence of the padded component count; the data side against
the model side (xcor.weighted_filter_reference); the mirror against np.linalg.lstsq; planted singular columns; and the ABI:
the struct's size, the constants, the exported symbol and the kernels in the code object."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bits import same_bits
from host_check import build_check

import many_cases as mc
import regress_cases as rc
import sysrem_cases as sc
from transit_amd import _abi, build, xcor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("regress_check", tmp_path_factory.mktemp("regress_check"))


def test_refusals_in_order_extents_merge_and_known_sets_under_sanitizers(check_exe):
    out = subprocess.run([check_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == ""                              # (no sanitizer report)
    lines = out.stdout.splitlines()
    last = lines[-1].split()
    assert last[0] == "ok" and int(last[1]) > 80, lines[-20:]
    assert not [line for line in lines if line.startswith("FAILED")]


def program(check_exe, path, data, w, seg, vec, nc=0):
    """the program's (coef, resid, nsingular) of one set under vectors [nseg, nexp, nvec], through the kernels of nc padded
    components (0: the count the library takes)"""
    nseg, nexp, nvec = vec.shape
    with open(path, "w") as f:
        f.write("%d %d %d %d %d\n%s\n" % (nexp, nseg, int(w is not None), nvec, nc, " ".join(str(int(x)) for x in seg)))
        for arr in (vec, data) + ((w,) if w is not None else ()):
            f.write(" ".join(float(x).hex() for x in np.asarray(arr).reshape(-1)) + "\n")
    out = subprocess.run([check_exe, "set", str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-4000:]
    lines = {w_[0]: w_[1:] for w_ in (line.split() for line in out.stdout.splitlines())}
    assert "FAILED" not in lines
    got = {k: np.array([float.fromhex(x) for x in lines[k]]) for k in ("coef", "data")}
    return got["coef"].reshape(nvec, data.shape[1]), got["data"].reshape(data.shape), int(lines["nsingular"][0])


def everywhere(vec, nseg):
    return np.ascontiguousarray(np.broadcast_to(vec[None, :, :], (nseg,) + vec.shape))


def sysrem_set(nexp, weighted):
    return sc.data_set(nexp, 70 + nexp), sc.edge_weights(nexp, 80 + nexp) if weighted else None


def check(check_exe, path, data, w, seg, vec, what, nc=0):
    want = xcor.regress_reference(data, w, seg, vec)
    got = program(check_exe, path, data, w, seg, vec, nc)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2], what
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all(), what
    return want


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nexp,nvec", [(7, 1), (7, 3), (7, 4), (7, 5), (12, 8), (12, 9), (rc.NEXP_16, 16)])
def test_the_programs_outputs_are_the_mirrors_bit_for_bit(check_exe, tmp_path, nexp, nvec, weighted):
    """sysrem_cases' segments of 1, 63, 64, 65, 200, 0, 7 and 400 pixels; the vectors are the airmass basis with seeded ones
    behind it"""
    data, w = sysrem_set(nexp, weighted)
    vec = everywhere(rc.given(nexp, nvec), len(sc.LENGTHS))
    what = "nexp %d, nvec %d, %s" % (nexp, nvec, "edge weights" if weighted else "no weights")
    coef, resid, nsing = check(check_exe, tmp_path / "set.txt", data, w, sc.SEG, vec, what)
    # what is singular: without weights nothing; with them every column with fewer live exposures than vectors (the column
    # masked everywhere among them) -- the necessary ones, counted here from the weights alone
    starved = np.zeros(sc.NPIX, dtype=bool) if w is None else np.count_nonzero(w > 0, axis=0) < nvec
    singular = np.all(coef == 0, axis=0) & np.all(resid == data, axis=0)
    assert nsing == np.count_nonzero(singular) and np.all(singular[starved]) and (weighted or nsing == 0), what
    assert nsing <= np.count_nonzero(starved) + 2, what          # (and next to none besides them)
    if weighted:
        assert np.all(coef[:, sc.MASKED_COL] == 0) and same_bits(resid[:, sc.MASKED_COL], data[:, sc.MASKED_COL]), what
    # least squares: the residuals are orthogonal to every vector under the weights, U^T diag(w) r = y - N c = 0, as far as
    # the rounding of y, N, the factor and the solve allows -- xcor.weighted_filter_bound's terms, to first order in u = 2^-53
    #   |y - N c|_j <= (nexp + 1) u Ya_j + ((nexp + 1) u Na + (3 n + 1) u S)_jk |c_k|,  Na_jk <= S_jk = sqrt(N_jj N_kk)
    # doubled for the second order, with (nexp + 1) u more for the sum that forms it here
    U = vec[0]
    ww = w if w is not None else np.ones_like(data)
    live = ~singular
    grad = np.einsum("vj,vp->jp", U, ww * resid)
    d = np.sqrt(np.einsum("vj,vp->jp", U * U, ww))
    scale = np.einsum("vj,vp->jp", np.abs(U), ww * np.abs(data)) + d * np.sum(d * np.abs(coef), axis=0)[None, :]
    bound = 2.0 * (3 * (nexp + 1) + 3 * nvec + 1) * 2.0 ** -53 * scale
    assert np.all(np.abs(grad[:, live]) <= bound[:, live]), (what, float(np.max(np.abs(grad[:, live]) / bound[:, live])))
    print("%s: largest |U^T W r| over its bound %.3f" % (what, float(np.max(np.abs(grad[:, live]) / bound[:, live]))))


@pytest.mark.parametrize("weighted", [False, True])
def test_vectors_that_differ_from_segment_to_segment(check_exe, tmp_path, weighted):
    data, w = sysrem_set(12, weighted)
    vec = rc.per_segment(len(sc.LENGTHS), 12, 5)
    want = check(check_exe, tmp_path / "set.txt", data, w, sc.SEG, vec, "per-segment vectors")
    # the mirror itself reads every segment's own vectors: segment 0's everywhere gives other bits in every other segment
    wrong = xcor.regress_reference(data, w, sc.SEG, vec[0])
    for s in (1, 2, 3, 4, 6, 7):
        k = slice(sc.SEG[s], sc.SEG[s + 1])
        assert not same_bits(want[1][:, k], wrong[1][:, k])
    assert same_bits(want[1][:, :1], wrong[1][:, :1])


@pytest.mark.parametrize("weighted", [False, True])
def test_the_long_orders(check_exe, tmp_path, weighted):
    """many_cases.long_set: orders of 1024, 1025, 0, 2049 and 7 pixels -- 16 and 32 whole tiles, and tiles of one lane behind them"""
    ms = mc.long_set()[0]
    w = ms.weight if weighted else None
    vec = everywhere(rc.airmass_vectors(ms.nexp, 2), ms.nseg)
    coef, resid, nsing = check(check_exe, tmp_path / "set.txt", ms.data, w, ms.seg_first, vec, "long orders")
    assert nsing == (1 if weighted else 0)


def test_the_bits_do_not_depend_on_the_padded_component_count(check_exe, tmp_path):
    data, w = sysrem_set(7, True)
    vec = everywhere(rc.given(7, 3), len(sc.LENGTHS))
    want = xcor.regress_reference(data, w, sc.SEG, vec)
    for nc in (4, 8, 16):
        got = program(check_exe, tmp_path / "set.txt", data, w, sc.SEG, vec, nc)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2], nc


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nexp,nvec", [(7, 3), (12, 9)])
def test_the_data_side_is_the_model_side(nexp, nvec, weighted):
    """the residuals are the weighted filter's values of the pairs (a, b) = (f0, 1) under gain 1 and the same vectors, bit for
    bit, in every column without a singular pivot (the filter gives NaN in the others, the regression f0)"""
    data, w = sysrem_set(nexp, weighted)
    vec = everywhere(rc.given(nexp, nvec), len(sc.LENGTHS))
    coef, resid, nsing = xcor.regress_reference(data, w, sc.SEG, vec)
    ob = xcor.Observed(sc.SEG, data, w, np.ones(sc.NPIX))
    val = xcor.weighted_filter_reference(np.stack([data, np.ones_like(data)], axis=-1), ob, xcor.WeightedFilter(vec))
    live = xcor.weighted_factor(ob, xcor.WeightedFilter(vec))[2]
    assert np.count_nonzero(~live) == nsing and np.isnan(val[:, ~live]).all() and not np.isnan(val[:, live]).any()
    assert same_bits(val[:, live], resid[:, live]) and same_bits(resid[:, ~live], data[:, ~live])


LSTSQ_DISTANCE = 1.85e-14     # measured (see the test's text)


def test_the_mirror_against_lstsq():
    """An independent check: np.linalg.lstsq of the sqrt(w)-scaled system, column by column, on a well-conditioned set --
    time_basis of degree 2 of the airmass, 12 exposures, sysrem_cases' data under the edge weights.  Measured here on the
    CPU (numpy with OpenBLAS): the mirror's largest distance to lstsq's coefficients, relative to the column's largest
    coefficient, is 1.85e-14 over the 799 fitted columns (LSTSQ_DISTANCE); the assertion allows 4 x that -- the margin covers
    another BLAS on another machine.  The device is never the yardstick."""
    nexp = 12
    data, w = sysrem_set(nexp, True)
    V = rc.airmass_vectors(nexp, 2)
    coef, resid, nsing = xcor.regress_reference(data, w, sc.SEG, V)
    worst = 0.0
    for p in range(sc.NPIX):
        if p == sc.MASKED_COL:
            continue
        sw = np.sqrt(w[:, p])
        c = np.linalg.lstsq(V * sw[:, None], data[:, p] * sw, rcond=None)[0]
        worst = max(worst, float(np.max(np.abs(coef[:, p] - c)) / np.max(np.abs(c))))
    print("largest relative distance of the mirror's coefficients to lstsq's: %.3e" % worst)
    assert nsing == 1 and worst <= 4 * LSTSQ_DISTANCE


@pytest.mark.parametrize("nc", [0, 16])
def test_planted_singular_columns(check_exe, tmp_path, nc):
    """a column live at fewer exposures than there are vectors, a column masked everywhere (sysrem_cases'), a segment whose
    vectors hold a duplicate: c = +0, r the bits of f0, and nsingular counts exactly these"""
    nexp, nvec, nseg = 12, 5, len(sc.LENGTHS)
    data = sc.data_set(nexp, 70 + nexp).copy()
    starved, dup_seg = int(sc.SEG[4]) + 7, 6
    assert starved != sc.MASKED_COL
    data[3, starved] = -0.0
    w = rc.starved_weights(sc.edge_weights(nexp, 80 + nexp), starved, nvec - 1)
    vec = rc.with_duplicate(rc.per_segment(nseg, nexp, nvec), dup_seg)
    coef, resid, nsing = check(check_exe, tmp_path / "set.txt", data, w, sc.SEG, vec, "planted", nc)
    dead = [starved, sc.MASKED_COL] + list(range(int(sc.SEG[dup_seg]), int(sc.SEG[dup_seg + 1])))
    assert nsing == len(dead) == 2 + sc.LENGTHS[dup_seg]
    assert np.all(coef[:, dead] == 0) and not np.signbit(coef[:, dead]).any()
    assert same_bits(resid[:, dead], data[:, dead]) and np.signbit(resid[3, starved])
    others = np.setdiff1d(np.arange(sc.NPIX), dead)
    assert np.all(np.any(coef[:, others] != 0, axis=0)) and not same_bits(resid[:, others], data[:, others])
    # one more live exposure and the starved column is fitted
    w2 = rc.starved_weights(w, starved, nvec)
    assert xcor.regress_reference(data, w2, sc.SEG, vec)[2] == nsing - 1


def test_time_basis():
    x = rc.airmass(12)
    T = xcor.time_basis(x, 2)
    t = (x - x.mean()) / np.abs(x - x.mean()).max()
    assert T.shape == (12, 3) and np.all(T[:, 0] == 1.0) and same_bits(T[:, 1], t) and same_bits(T[:, 2], t ** 2)
    assert np.abs(T).max() == 1.0 and np.linalg.cond(T) < 10.0
    assert np.all(xcor.time_basis(np.full(5, 1.3), 1) == np.array([1.0, 0.0])[None, :])
    assert xcor.time_basis(x, 0).shape == (12, 1)
    for bad in ((x, -1), ([1.0, float("nan")], 1)):
        with pytest.raises(ValueError):
            xcor.time_basis(*bad)
    with pytest.raises(ValueError):
        xcor.regress_reference(np.ones((3, 5)), None, [0, 5], np.ones((4, 2)))
    with pytest.raises(ValueError):
        xcor.regress_reference(np.ones((3, 5)), None, [0, 5], np.full((3, 2), np.inf))


def test_abi_struct_constants_symbol_and_kernels():
    assert ctypes.sizeof(_abi.TrxRegress) == 40
    assert [n for n, _ in _abi.TrxRegress._fields_] == ["nvec", "nfit", "niter", "inject", "p0", "p1", "vectors"]
    assert _abi.TrxRegress.vectors.offset == 32 and _abi.TrxRegress.p0.offset == 16
    assert (_abi.FILTER_MAX, _abi.SYSREM_MAX_ITER, _abi.WFILTER_PIVOT) == (16, 64, 2.0 ** -26)
    txt = open(os.path.join(ROOT, "include", "transit_hip.h")).read()
    for line in ("#define TRX_FILTER_MAX 16", "#define TRX_SYSREM_MAX_ITER 64", "#define TRX_WFILTER_PIVOT 0x1p-26", "#define TRX_ABI_VERSION 5",
                 "} trx_regress;               /* 40 bytes */"):
        assert line in txt, line
    path = build.lib_path("libtransit_hip.so")
    if not os.path.exists(path):
        build.build_hip()
    lib = ctypes.CDLL(path)
    assert hasattr(lib, "trx_regress_observed")
    lib.trx_abi_version.restype = ctypes.c_int
    assert lib.trx_abi_version() == 5
    blob = open(path, "rb").read()
    for nc in (4, 8, 16):
        assert b"k_regress_colsILi%dEE" % nc in blob, nc
    # refused without a handle, before anything is touched
    _abi.bind(lib, _abi.HIP_HEADER, "trx_")
    assert lib.trx_regress_observed(None, None, None, None, 0, None, None, None, None, None, None, None, None) == -1
