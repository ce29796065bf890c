"""Weighing the observed set by its columns' scatter without a device: the refusals, the tiles, the extents and the
arithmetic of transit_amd/csrc/trx_scatter.h through tests/scatter_check.cpp, a stand-alone program over exact-size heap
arrays under -fsanitize=address,undefined that walks a whole set the way the kernels do; its var, med and w' held bit for
bit against xcor.scatter_reference, the numpy mirror; the planted columns of scatter_cases (the ties at the median rank, the
constant and the masked column, the five noisy columns and the margin of their clip); the mirror's own properties (weights
None = weights 1, the median against np.sort, the variance against np.var); and the ABI: the struct's size, the constants,
the exported symbol and the kernels in the code object."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bits import same_bits
from host_check import build_check

import many_cases as mc
import scatter_cases as cs
from transit_amd import _abi, build, xcor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("scatter_check", tmp_path_factory.mktemp("scatter_check"))


def test_refusals_extents_tiles_and_known_sets_under_sanitizers(check_exe):
    out = subprocess.run([check_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == ""                              # (no sanitizer report)
    lines = out.stdout.splitlines()
    last = lines[-1].split()
    assert last[0] == "ok" and int(last[1]) > 80, lines[-20:]
    assert not [line for line in lines if line.startswith("FAILED")]


_MIRROR = {}


def mirror(nexp, weighted, kind, clip, min_live):
    """(data, weight, (var, med, keep, w')) of the shared set, computed once per case"""
    key = (nexp, weighted, kind, clip, min_live)
    if key not in _MIRROR:
        data, w, _ = cs.the_set(nexp, weighted)
        _MIRROR[key] = (data, w, xcor.scatter_reference(data, w, cs.SEG, kind, clip, min_live))
    return _MIRROR[key]


def program_is_the_mirror(check_exe, path, data, w, seg, kind, clip, min_live, want):
    """the program's var, med, w' and nmasked of one set under one call against the mirror's, bit for bit"""
    var, med, keep, out_w = want
    nexp = data.shape[0]
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %s\n%s\n" % (nexp, kind, min_live, len(seg) - 1, int(w is not None), float(clip).hex(), " ".join(str(int(x)) for x in seg)))
        for arr in (data,) + ((w,) if w is not None else ()):
            f.write(" ".join(float(x).hex() for x in arr.reshape(-1)) + "\n")
    out = subprocess.run([check_exe, "set", str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-4000:]
    lines = {w_[0]: w_[1:] for w_ in (line.split() for line in out.stdout.splitlines())}
    assert "FAILED" not in lines
    got = {k: np.array([float.fromhex(x) for x in lines[k]]) for k in ("var", "med", "w")}
    assert same_bits(got["var"], var)
    assert same_bits(got["med"], med)
    assert same_bits(got["w"].reshape(out_w.shape), out_w)
    assert int(lines["nmasked"][0]) == np.count_nonzero((var > 0) & ~keep)


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("clip", cs.CLIPS)
@pytest.mark.parametrize("kind", cs.KINDS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nexp", [7, 12])
def test_the_programs_variances_medians_and_weights_are_the_mirrors_bit_for_bit(check_exe, tmp_path, nexp, weighted, kind, clip, full):
    min_live = nexp if full else 2
    data, w, (var, med, keep, out_w) = mirror(nexp, weighted, kind, clip, min_live)
    program_is_the_mirror(check_exe, tmp_path / "set.txt", data, w, cs.SEG, kind, clip, min_live, (var, med, keep, out_w))
    live = var > 0
    # the edges: the empty segment's median is +0, the one-pixel segment's is its column's variance; the planted dead columns
    # (+0 where that column is dead)
    assert med[5] == 0 and not np.signbit(med[5]) and same_bits(med[0], var[0]) and (var[0] > 0 or (weighted and full))
    assert var[cs.CONSTANT_COL] == 0 and not keep[cs.CONSTANT_COL] and np.all(out_w[:, cs.CONSTANT_COL] == 0)
    assert np.isfinite(var).all() and np.isfinite(out_w).all() and not np.signbit(out_w).any()
    if weighted:
        assert var[cs.MASKED_COL] == 0 and np.all(out_w[:, cs.MASKED_COL] == 0)
        assert np.all(out_w[w == 0] == 0) and np.all(out_w[:, keep][w[:, keep] > 0] > 0)
        # (under the edge weights 5 % of the entries are masked: min_live = nexp leaves the columns without one)
        assert np.array_equal(live, (np.count_nonzero(w > 0, axis=0) >= min_live) & (np.arange(cs.NPIX) != cs.CONSTANT_COL))
    else:
        assert np.count_nonzero(live) == cs.NPIX - 1
    if clip == 0:
        assert np.array_equal(keep, live)
    if kind == xcor.SCATTER_MASK:
        assert same_bits(out_w, np.where(keep[None, :], np.ones_like(data) if w is None else w, 0.0))
    else:
        assert same_bits(out_w[:, keep].max(axis=0), 1.0 / var[keep])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nexp", [7, 12])
def test_the_planted_ties_straddle_the_median_rank(nexp, weighted):
    data, w, (var, med, keep, _) = mirror(nexp, weighted, xcor.SCATTER_VARIANCE, 0.0, 2)
    ties = cs.the_set(nexp, weighted)[2]
    for s, (a, b) in zip(cs.TIE_SEGS, ties):
        order = cs.ranked(var, s)
        m = order.size
        # two identical columns at the ranks (m - 1) // 2 and the next: the lower pixel first, and the median is their variance
        assert a != b and same_bits(data[:, a], data[:, b]) and same_bits(var[a], var[b])
        assert sorted(int(p) for p in order[(m - 1) // 2:(m - 1) // 2 + 2]) == sorted((a, b))
        assert int(order[(m - 1) // 2]) == min(a, b) and same_bits(med[s], var[a])
        assert np.count_nonzero(var[cs.SEG[s]:cs.SEG[s + 1]] == var[a]) == 2
        if not weighted:
            assert m == cs.LENGTHS[s] and m % 2 == (1 if s == 3 else 0)      # an odd and an even number of live columns


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nexp", [7, 12])
def test_the_clip_of_three_removes_exactly_the_noisy_columns_with_a_margin(nexp, weighted):
    """The precondition of every clip = 3 case: the five columns of 10 x the noise are the ones removed, and no live column's
    var / med lies within 5 % of 9 -- the clipped set cannot flip on a last bit."""
    for min_live in (2, nexp):
        var, med, keep, _ = mirror(nexp, weighted, xcor.SCATTER_MASK, 3.0, min_live)[2]
        clipped, margin = cs.clip_margin(var, med, keep)
        print("nexp %d, %s, min_live %d: clipped %s, nearest var / (9 med) is %.3f away from 1" % (nexp, "edge weights" if weighted else "no weights", min_live, clipped, margin))
        want = tuple(p for p in cs.NOISY_COLS if var[p] > 0)
        assert clipped == want and margin > 0.05
        if min_live == 2:
            assert want == cs.NOISY_COLS


@pytest.mark.parametrize("kind", cs.KINDS)
@pytest.mark.parametrize("nexp", [7, 12])
def test_weights_none_are_weights_one(nexp, kind):
    data, _, got = mirror(nexp, False, kind, 3.0, 2)
    ones = xcor.scatter_reference(data, np.ones_like(data), cs.SEG, kind, 3.0, 2)
    for a, b in zip(got, ones):
        assert same_bits(a, b)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nexp", [7, 12])
def test_the_median_is_the_sorted_live_variances_lower_middle(nexp, weighted):
    for min_live in (2, nexp):
        var, med, _, _ = mirror(nexp, weighted, xcor.SCATTER_VARIANCE, 0.0, min_live)[2]
        for s in range(len(cs.LENGTHS)):
            x = var[cs.SEG[s]:cs.SEG[s + 1]]
            x = x[x > 0]
            assert same_bits(med[s], np.sort(x)[(x.size - 1) // 2] if x.size else 0.0)


def test_the_variance_against_numpys():
    """The mirror's two passes in exposure order against np.var(ddof=1), whose sums are numpy's own (pairwise): the two differ
    by the rounding of the sums.  The largest relative difference over the shared sets (7 and 12 exposures, with and without
    the edge weights) was measured at 4.6e-16 -- a few units in the last place --; the bound 1e-13 leaves a factor above 100
    for another platform's summation order."""
    worst = 0.0
    for nexp in (7, 12):
        for weighted in (False, True):
            data, w, (var, _, _, _) = mirror(nexp, weighted, xcor.SCATTER_VARIANCE, 0.0, 2)
            for p in np.flatnonzero(var > 0):
                col = data[:, p] if w is None else data[w[:, p] > 0, p]
                worst = max(worst, abs(var[p] - np.var(col, ddof=1)) / var[p])
    print("largest relative |mirror - np.var(ddof=1)|: %.2e" % worst)
    assert worst < 1e-13


# ---- the long orders of many_cases.long_set: 1024, 1025, 0, 2049 and 7 pixels -- one staging trip exactly, a second trip of
# one value, three trips; the ties across trips, the noisy columns in the one-column tile and at the 1023 | 1024 border
def long_mirror(weighted, kind, clip, min_live):
    """(set, planted, weights or None, the mirror's four) of the long set whose ties are planted for this weighting"""
    key = ("long", weighted, kind, clip, min_live)
    if key not in _MIRROR:
        ms, pl = mc.long_set(weighted)
        w = ms.weight if weighted else None
        _MIRROR[key] = (ms, pl, w, xcor.scatter_reference(ms.data, w, ms.seg_first, kind, clip, min_live))
    return _MIRROR[key]


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("clip", cs.CLIPS)
@pytest.mark.parametrize("kind", cs.KINDS)
@pytest.mark.parametrize("weighted", [False, True])
def test_the_programs_variances_medians_and_weights_on_the_long_orders(check_exe, tmp_path, weighted, kind, clip, full):
    """the kernels' own source on the CPU, kScatLds = 1024 as on the device: the 1025- and the 2049-pixel segment take two and
    three staging trips, the last of one value padded to kScatTrip; every (kind, clip, min_live) of the 800-pixel test"""
    min_live = mc.LONG_NEXP if full else 2
    ms, pl, w, want = long_mirror(weighted, kind, clip, min_live)
    program_is_the_mirror(check_exe, tmp_path / "set.txt", ms.data, w, ms.seg_first, kind, clip, min_live, want)
    var, med, keep, out_w = want
    assert med[2] == 0 and not np.signbit(med[2]) and np.isfinite(var).all() and np.isfinite(out_w).all() and not np.signbit(out_w).any()
    if min_live == 2:
        for s, a, b in pl.ties:
            assert same_bits(med[s], var[a]) and same_bits(var[a], var[b])
    elif weighted:                                               # an exposure is masked over the whole 1025-pixel segment: no column of 12
        assert med[ms.masked_seg] == 0 and not var[ms.segment(ms.masked_seg)].any()


@pytest.mark.parametrize("weighted", [False, True])
def test_the_median_is_the_sorted_live_variances_lower_middle_on_the_long_orders(weighted):
    for min_live in (2, mc.LONG_NEXP):
        ms, _, _, (var, med, _, _) = long_mirror(weighted, xcor.SCATTER_VARIANCE, 0.0, min_live)
        for s in range(ms.nseg):
            x = var[ms.segment(s)]
            x = x[x > 0]
            assert same_bits(med[s], np.sort(x)[(x.size - 1) // 2] if x.size else 0.0)


def test_the_variance_against_numpys_on_the_long_orders():
    """test_the_variance_against_numpys' rule -- 1e-13 of the variance -- over the 4105 columns of the long set, with and
    without the weights"""
    worst = 0.0
    for weighted in (False, True):
        ms, _, w, (var, _, _, _) = long_mirror(weighted, xcor.SCATTER_VARIANCE, 0.0, 2)
        for p in np.flatnonzero(var > 0):
            col = ms.data[:, p] if w is None else ms.data[w[:, p] > 0, p]
            worst = max(worst, abs(var[p] - np.var(col, ddof=1)) / var[p])
    print("long orders: largest relative |mirror - np.var(ddof=1)|: %.2e" % worst)
    assert worst < 1e-13


def test_the_mirror_refuses_what_it_does_not_define():
    with pytest.raises(ValueError):
        xcor.scatter_reference(np.zeros(5), None, [0, 5], xcor.SCATTER_MASK)
    with pytest.raises(ValueError):
        xcor.scatter_reference(np.zeros((3, 5)), None, [0, 5], xcor.SCATTER_NONE)


def test_abi_struct_constants_symbol_and_kernels():
    assert ctypes.sizeof(_abi.TrxScatter) == 16
    assert (_abi.SCATTER_NONE, _abi.SCATTER_VARIANCE, _abi.SCATTER_MASK) == (0, 1, 2)
    assert (xcor.SCATTER_NONE, xcor.SCATTER_VARIANCE, xcor.SCATTER_MASK) == (0, 1, 2)
    txt = open(os.path.join(ROOT, "include", "transit_hip.h")).read()
    for line in ("#define TRX_SCATTER_NONE     0", "#define TRX_SCATTER_VARIANCE 1", "#define TRX_SCATTER_MASK     2"):
        assert line in txt
    path = build.lib_path("libtransit_hip.so")
    if not os.path.exists(path):
        build.build_hip()
    lib = ctypes.CDLL(path)
    assert hasattr(lib, "trx_weigh_observed")
    lib.trx_abi_version.restype = ctypes.c_int
    assert lib.trx_abi_version() == 5
    blob = open(path, "rb").read()
    for k in (b"k_scatter_cols", b"k_scatter_median", b"k_scatter_weights"):
        assert k in blob, k
    # refused without a handle, before anything is touched
    _abi.bind(lib, _abi.HIP_HEADER, "trx_")
    assert lib.trx_weigh_observed(None, None, None, None, None, None, None) == -1
