"""The host side of the moment runs (transit_amd/xcor.py) against sums written out by hand and against the quantities
computed directly from f, g, w, and the library's new entry points as far as they go without a device (no GPU).

The reductions from moments are compared with the direct ones to 1e-12 relative to the sums of ABSOLUTE terms: a
moment is a sum whose rounding error scales with the sum of its |terms|, and chi2 / the central moments combine
moments with cancellation, so that is the scale their difference from a direct evaluation has.  For the ratios (ccf)
and the logarithm (loglike_bl19) that bound is carried through to first order."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from transit_amd import _abi, build, xcor


def test_segments_and_observed():
    assert xcor.segments([1, 63, 0, 7]).tolist() == [0, 1, 64, 64, 71]
    assert xcor.segments([]).tolist() == [0]
    assert xcor.segments([3]).dtype == np.int64
    with pytest.raises(ValueError):
        xcor.segments([2, -1])
    ob = xcor.Observed(xcor.segments([2, 1]), [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], gain=[1.0, 2.0, 3.0])
    assert (ob.nexp, ob.nseg, ob.npix) == (2, 2, 3)
    c = ob.to_c()
    assert C.sizeof(_abi.TrxObserved) == 40
    assert (c.nexp, c.nseg, c.seg_first[2], c.data[4], c.gain[2]) == (2, 2, 3, 5.0, 3.0) and not c.weight
    with pytest.raises(ValueError):
        xcor.Observed([0, 3], [1.0, 2.0, 3.0])                           # data is [nexp][npix]
    with pytest.raises(ValueError):
        xcor.Observed([0, 3], [[1.0, 2.0, 3.0]], weight=[[1.0, 1.0]])
    with pytest.raises(ValueError):
        xcor.Observed([0, 3], [[1.0, 2.0, 3.0]], gain=[1.0])
    assert xcor.NMOMENT == 7


def test_reference_against_sums_written_out():
    # one exposure, six pixels: segments [0, 3), [3, 3) (empty), [3, 6)
    #   pixel      0      1      2    |   3      4      5
    #   a          2      3      9    |   1      5      4
    #   b          4      0      3    |   2      2      8
    #   gain       2      1      1    |   3      1      2
    #   g          1     (b=0)   3    |  1.5    2.5     1
    #   f          3      7     -1    |   2      4     -2
    #   w          2      5      1    |   4      0      1
    pairs = np.array([[[2.0, 4.0], [3.0, 0.0], [9.0, 3.0], [1.0, 2.0], [5.0, 2.0], [4.0, 8.0]]])
    ob = xcor.Observed(xcor.segments([3, 0, 3]), [[3.0, 7.0, -1.0, 2.0, 4.0, -2.0]], [[2.0, 5.0, 1.0, 4.0, 0.0, 1.0]],
                       [2.0, 1.0, 1.0, 3.0, 1.0, 2.0])
    m = xcor.reference(pairs, ob)
    assert m.shape == (1, 3, 7)
    # segment 0: pixels 0 and 2 (pixel 1 has b = 0)
    assert m[0, 0].tolist() == [2.0, 2 + 1, 2 * 1 + 1 * 3, 2 * 1 + 1 * 9, 2 * 3 + 1 * -1, 2 * 3 * 1 + 1 * -1 * 3, 2 * 9 + 1 * 1]
    # segment 1: empty -- seven zeros, none of them negative
    assert m[0, 1].tolist() == [0.0] * 7 and not np.any(np.signbit(m[0, 1]))
    # segment 2: pixels 3 and 5 (pixel 4 is masked, w = 0)
    assert m[0, 2].tolist() == [2.0, 4 + 1, 4 * 1.5 + 1 * 1, 4 * 2.25 + 1 * 1, 4 * 2 + 1 * -2, 4 * 2 * 1.5 + 1 * -2 * 1, 4 * 4 + 1 * 4]
    ab = xcor.abs_reference(pairs, ob)
    assert ab[0, 0].tolist() == [2.0, 3.0, 5.0, 11.0, 2 * 3 + 1 * 1, 2 * 3 * 1 + 1 * 1 * 3, 19.0]
    assert ab[0, 2].tolist() == [2.0, 5.0, 7.0, 10.0, 4 * 2 + 1 * 2, 4 * 2 * 1.5 + 1 * 2 * 1, 20.0]
    # no weights, no gain: w = 1 and g = a / b; a segment whose pixels all have b = 0 is seven zeros too
    ob1 = xcor.Observed(xcor.segments([1, 2, 3]), ob.data)
    m1 = xcor.reference(pairs, ob1)
    assert m1[0, 0].tolist() == [1.0, 1.0, 0.5, 0.25, 3.0, 1.5, 9.0]
    assert m1[0, 1].tolist() == [1.0, 1.0, 3.0, 9.0, -1.0, -3.0, 1.0]
    ob2 = xcor.Observed(xcor.segments([1, 1, 4]), ob.data)
    assert xcor.reference(pairs, ob2)[0, 1].tolist() == [0.0] * 7
    with pytest.raises(ValueError):
        xcor.reference(pairs[:, :5], ob)


def direct(f, g, w):
    """(n, W, mean-subtracted s_f^2, s_g^2, R) of one row, the means subtracted before anything is squared"""
    sw = math.fsum(w)
    mf, mg = math.fsum(w * f) / sw, math.fsum(w * g) / sw
    return (len(f), sw, math.fsum(w * (f - mf) ** 2) / sw, math.fsum(w * (g - mg) ** 2) / sw,
            math.fsum(w * (f - mf) * (g - mg)) / sw)


def test_reductions_from_moments_against_direct_evaluation():
    rng = np.random.default_rng(7)
    nexp, lens = 5, [1, 2, 17, 0, 300, 64]
    seg = xcor.segments(lens)
    npix = int(seg[-1])
    b = rng.uniform(0.5, 2.0, (nexp, npix))
    a = b * (1.0 + 0.2 * rng.standard_normal((nexp, npix)))
    b[:, 5] = 0.0                                                         # a pixel off the grid
    pairs = np.stack([a, b], axis=-1)
    f = 1.0 + 0.1 * rng.standard_normal((nexp, npix)) - 0.6
    w = rng.uniform(0.5, 2.0, (nexp, npix))
    w[rng.random((nexp, npix)) < 0.05] = 0.0
    gain = rng.uniform(0.5, 1.5, npix)
    ob = xcor.Observed(seg, f, w, gain)
    mom, amom = xcor.reference(pairs, ob), xcor.abs_reference(pairs, ob)
    tol = 1e-12
    worst = {"chi2": 0.0, "ccf": 0.0, "loglike": 0.0}
    seen_nan = 0
    for v in range(nexp):
        for s in range(len(lens)):
            k = np.arange(seg[s], seg[s + 1])
            k = k[(b[v, k] > 0) & (w[v, k] > 0)]
            fk, wk, gk = f[v, k], w[v, k], gain[k] * (a[v, k] / b[v, k])
            assert mom[v, s, 0] == k.size
            for ca, cb in ((1.0, 0.0), (0.7, -0.2), (-1.3, 0.05)):
                want = math.fsum(wk * (fk - ca * gk - cb) ** 2)
                scale = math.fsum(wk * (np.abs(fk) + abs(ca) * np.abs(gk) + abs(cb)) ** 2)
                assert scale == pytest.approx(xcor.chi2(amom, -abs(ca), -abs(cb))[v, s], rel=1e-13)
                got = xcor.chi2(mom, ca, cb)[v, s]
                assert abs(got - want) <= tol * scale, (v, s, ca, cb)
                if scale:
                    worst["chi2"] = max(worst["chi2"], abs(got - want) / scale)
            cc, ll = xcor.ccf(mom)[v, s], xcor.loglike_bl19(mom, 0.8)[v, s]
            if k.size < 2:
                assert math.isnan(cc) and math.isnan(ll)
                seen_nan += 1
                continue
            n, sw, sf2, sg2, r = direct(fk, gk, wk)
            # the sums of absolute terms behind the three central moments
            mf, mg = amom[v, s, xcor.WF] / sw, amom[v, s, xcor.WG] / sw
            sf2_abs, sg2_abs = amom[v, s, xcor.WFF] / sw + mf * mf, amom[v, s, xcor.WGG] / sw + mg * mg
            r_abs = amom[v, s, xcor.WFG] / sw + mf * mg
            want = r / math.sqrt(sf2 * sg2)
            bound = tol * (r_abs / math.sqrt(sf2 * sg2) + abs(want) * 0.5 * (sf2_abs / sf2 + sg2_abs / sg2))
            assert abs(cc - want) <= bound, (v, s, cc, want)
            worst["ccf"] = max(worst["ccf"], abs(cc - want) / bound * tol)
            arg = sf2 - 2 * 0.8 * r + 0.64 * sg2
            want = -0.5 * n * math.log(arg)
            bound = tol * 0.5 * n * (sf2_abs + 1.6 * r_abs + 0.64 * sg2_abs) / arg
            assert abs(ll - want) <= bound, (v, s, ll, want)
            worst["loglike"] = max(worst["loglike"], abs(ll - want) / bound * tol)
    print("worst error over its sum of absolute terms:", worst)
    assert seen_nan >= 2 * nexp                                           # the segments of 1 and of 0 pixels, at least
    # the summing wrappers: chi2 over every row, the other two over the rows that have a value
    assert xcor.chi2_sum(mom, 0.7, -0.2) == pytest.approx(float(np.sum(xcor.chi2(mom, 0.7, -0.2))), rel=1e-15)
    cc = xcor.ccf(mom)
    assert np.isnan(cc).sum() == seen_nan
    assert xcor.ccf_sum(mom) == pytest.approx(float(np.sum(cc[~np.isnan(cc)])), rel=1e-15)
    ll = xcor.loglike_bl19(mom, 0.8)
    assert math.isfinite(xcor.loglike_bl19_sum(mom, 0.8))
    assert xcor.loglike_bl19_sum(mom, 0.8) == pytest.approx(float(np.sum(ll[~np.isnan(ll)])), rel=1e-15)


def test_zero_variance_rows_have_no_coefficient():
    # g constant over the segment: s_g^2 = 0
    pairs = np.array([[[2.0, 1.0], [4.0, 2.0], [6.0, 3.0]]])
    ob = xcor.Observed([0, 3], [[1.0, 2.0, 4.0]])
    mom = xcor.reference(pairs, ob)
    assert mom[0, 0, 0] == 3 and math.isnan(xcor.ccf(mom)[0, 0]) and math.isnan(xcor.loglike_bl19(mom)[0, 0])
    assert xcor.ccf_sum(mom) == 0.0 and xcor.loglike_bl19_sum(mom) == 0.0
    assert xcor.chi2(mom)[0, 0] == (1 - 2) ** 2 + (2 - 2) ** 2 + (4 - 2) ** 2
    # a perfect match: ccf = 1, and chi2 = 0 at a = 1
    ob = xcor.Observed([0, 3], [[1.0, 2.0, 4.0]])
    mom = xcor.reference(np.array([[[1.0, 1.0], [2.0, 1.0], [4.0, 1.0]]]), ob)
    assert xcor.ccf(mom)[0, 0] == pytest.approx(1.0, rel=1e-15) and xcor.chi2(mom)[0, 0] == 0.0


def test_library_exports_and_refuses_without_a_handle():
    path = build.lib_path("libtransit_hip.so")
    if not os.path.exists(path):
        build.build_hip()
    lib = C.CDLL(path)
    for name in ("trx_set_observed", "trx_run_moments", "trx_batch_set_observed", "trx_run_batch_moments"):
        assert hasattr(lib, name), name
    _abi.bind(lib, _abi.HIP_HEADER, "trx_")
    ob = xcor.Observed([0, 2], [[1.0, 2.0]])
    assert lib.trx_set_observed(None, C.byref(ob.to_c())) == -1
    assert lib.trx_set_observed(None, None) == -1
    assert lib.trx_batch_set_observed(None, C.byref(ob.to_c())) == -1
    mom, sh = np.zeros((1, 1, 7)), np.ones(1)
    assert lib.trx_run_moments(None, None, None, None, 1, sh.ctypes.data_as(_abi.c_double_p),
                               mom.ctypes.data_as(_abi.c_double_p), None) == -1
    assert lib.trx_run_batch_moments(None, 0, None, None, 1, None, None) == -1
    blob = open(path, "rb").read()
    assert b"k_pixel_moments" in blob
