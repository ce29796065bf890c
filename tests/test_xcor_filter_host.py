"""The host side of the filtered moment runs (transit_amd/xcor.py: Filter, svd_filter, filter_reference,
filter_abs_reference, reference_values) against a case worked by hand and against the properties of the definition,
and the library's new entry points as far as they go without a device (no GPU).

Tolerance of a filtered value, relative to filter_abs_reference A = |g| + |back| (|fwd| |g|):
(nexp + ncomp + 8) * 2^-52 -- two roundings in g, nexp products and sums in a coefficient, ncomp in the projection,
one subtraction, doubled for the reference's own rounding; derived, not measured."""
import ctypes as C
import os

import numpy as np
import pytest

from transit_amd import _abi, build, xcor

EPS = 2.0 ** -52


def tolerance(nexp, ncomp):
    return (nexp + ncomp + 8) * EPS


def test_filter_and_its_c_form():
    fwd = np.arange(24.0).reshape(2, 3, 4)
    F = xcor.Filter(fwd, fwd.transpose(0, 2, 1))
    assert (F.nseg, F.ncomp, F.nexp) == (2, 3, 4) and F.back.flags.c_contiguous
    c = F.to_c()
    assert C.sizeof(_abi.TrxFilter) == 24 and _abi.FILTER_MAX == 16
    assert (c.ncomp, c.pad, c.fwd[5], c.back[5]) == (3, 0, 5.0, F.back.ravel()[5])
    with pytest.raises(ValueError):
        xcor.Filter(fwd, fwd)                                             # back is [nseg][nexp][ncomp]
    with pytest.raises(ValueError):
        xcor.Filter(fwd[0], fwd[0].T)
    ob = xcor.Observed([0, 2], [[1.0, 2.0]] * 3)
    with pytest.raises(ValueError):
        xcor.filter_reference(np.ones((3, 2, 2)), ob, F)                  # another nseg and nexp


def test_three_exposures_two_pixels_by_hand():
    #   exposure       0      1      2
    #   pixel 0   a    2      4      6       pixel 1   a    4      0      8
    #             b    1      2      2                 b    2      1      4
    #   gain 1    g    2      2      3       gain 2    g    4      0      4
    # one segment, one component: fwd = (1/2, 1/4, 1/4), back = (1, 2, 0)
    #   c(pixel 0) = 1 + 1/2 + 3/4 = 9/4     r = (9/4, 9/2, 0)     g' = (-1/4, -5/2, 3)
    #   c(pixel 1) = 2 + 0 + 1 = 3           r = (3, 6, 0)         g' = (1, -6, 4)
    pairs = np.array([[[2.0, 1.0], [4.0, 2.0]], [[4.0, 2.0], [0.0, 1.0]], [[6.0, 2.0], [8.0, 4.0]]])
    f = np.array([[1.0, 2.0], [3.0, -1.0], [0.5, 2.0]])
    ob = xcor.Observed([0, 2], f, gain=[1.0, 2.0])
    F = xcor.Filter([[[0.5, 0.25, 0.25]]], [[[1.0], [2.0], [0.0]]])
    got = xcor.filter_reference(pairs, ob, F)
    assert got.tolist() == [[-0.25, 1.0], [-2.5, -6.0], [3.0, 4.0]]
    assert xcor.filter_abs_reference(pairs, ob, F).tolist() == [[2 + 2.25, 4 + 3.0], [2 + 4.5, 0 + 6.0], [3 + 0.0, 4 + 0.0]]
    m = xcor.reference_values(got, ob)
    assert m.shape == (3, 1, 7)
    assert m[0, 0].tolist() == [2.0, 2.0, -0.25 + 1, 0.0625 + 1, 1.0 + 2, -0.25 + 2, 1.0 + 4]
    assert m[1, 0].tolist() == [2.0, 2.0, -2.5 - 6, 6.25 + 36, 3.0 - 1, -7.5 + 6, 9.0 + 1]
    assert m[2, 0].tolist() == [2.0, 2.0, 3.0 + 4, 9.0 + 16, 0.5 + 2, 1.5 + 8, 0.25 + 4]
    assert xcor.abs_reference_values(got, ob)[1, 0].tolist() == [2.0, 2.0, 8.5, 42.25, 4.0, 13.5, 10.0]
    # with weights: a masked pixel has a value and counts in no moment
    obw = xcor.Observed([0, 2], f, [[2.0, 0.0], [1.0, 1.0], [0.0, 3.0]], [1.0, 2.0])
    assert np.array_equal(xcor.filter_reference(pairs, obw, F), got)      # (the weights take no part in the projection)
    mw = xcor.reference_values(got, obw)
    assert mw[0, 0].tolist() == [1.0, 2.0, -0.5, 0.125, 2.0, -0.5, 2.0]
    assert mw[2, 0].tolist() == [1.0, 3.0, 12.0, 48.0, 6.0, 24.0, 12.0]
    with pytest.raises(ValueError):
        xcor.reference_values(got[:, :1], ob)


def test_svd_filter_is_an_orthonormal_basis_per_segment():
    rng = np.random.default_rng(5)
    data = rng.standard_normal((7, 40))
    seg = xcor.segments([10, 0, 28, 2])
    F = xcor.svd_filter(data, seg, 3)
    assert (F.nseg, F.ncomp, F.nexp) == (4, 3, 7)
    eye = np.eye(3)
    for s in (0, 2):
        assert np.max(np.abs(F.fwd[s] @ F.back[s] - eye)) <= 16 * EPS
        assert np.array_equal(F.fwd[s], F.back[s].T)
        u = np.linalg.svd(data[:, seg[s]:seg[s + 1]], full_matrices=False)[0]
        assert np.array_equal(F.back[s], u[:, :3])
    assert not F.fwd[1].any() and not F.back[1].any()                     # an empty segment: zeros
    # two pixels have two singular vectors: the third component is padding
    assert np.max(np.abs(F.fwd[3] @ F.back[3] - np.diag([1.0, 1.0, 0.0]))) <= 16 * EPS
    assert not F.back[3][:, 2].any() and not F.fwd[3][2].any()


@pytest.mark.parametrize("ncomp", [1, 3, 7, 16])
def test_a_model_inside_the_basis_filters_to_zero(ncomp):
    rng = np.random.default_rng(11)
    nexp, lens = (7 if ncomp <= 7 else 20), [1, 63, 0, 130]
    seg = xcor.segments(lens)
    npix = int(seg[-1])
    data = rng.standard_normal((nexp, npix))
    F = xcor.svd_filter(data, seg, ncomp)
    gain = rng.uniform(0.5, 1.5, npix)
    ob = xcor.Observed(seg, data, gain=gain)
    tol = tolerance(nexp, ncomp)
    worst = 0.0
    for j in range(ncomp):
        # u_j[v] * h[p], u_j the segment's own j-th basis vector (zero where the segment has fewer): g = gain * (a / b)
        h = rng.uniform(0.5, 2.0, npix) * rng.choice([-1.0, 1.0], npix)
        b = rng.uniform(0.5, 2.0, (nexp, npix))
        u = np.concatenate([np.repeat(F.back[s][:, j:j + 1], lens[s], axis=1) for s in range(len(lens))], axis=1)
        pairs = np.stack([u * h[None, :] * b, b], axis=-1)
        got = xcor.filter_reference(pairs, ob, F)
        scale = xcor.filter_abs_reference(pairs, ob, F)
        assert not np.isnan(got).any() and np.count_nonzero(scale) >= nexp * 190
        assert np.all(np.abs(got) <= tol * scale), (ncomp, j)
        worst = max(worst, float(np.max(np.abs(got[scale > 0]) / scale[scale > 0])))
    print("ncomp %d: worst |g'| / A %.3e = %.2f of the tolerance %.3e" % (ncomp, worst, worst / tol, tol))


def test_a_column_off_the_grid_at_one_exposure_is_dead():
    rng = np.random.default_rng(3)
    nexp, npix = 5, 12
    b = rng.uniform(0.5, 2.0, (nexp, npix))
    a = b * rng.uniform(0.5, 2.0, (nexp, npix))
    b[2, 4] = 0.0
    a[2, 4] = 0.0
    pairs = np.stack([a, b], axis=-1)
    seg = xcor.segments([6, 6])
    f = rng.standard_normal((nexp, npix))
    ob = xcor.Observed(seg, f)
    F = xcor.svd_filter(f, seg, 2)
    got = xcor.filter_reference(pairs, ob, F)
    assert np.isnan(got[:, 4]).all() and np.isnan(got).sum() == nexp
    assert np.isnan(xcor.filter_abs_reference(pairs, ob, F)[:, 4]).all()
    m = xcor.reference_values(got, ob)
    assert np.array_equal(m[:, :, 0], [[5.0, 6.0]] * nexp)
    # ... while the unfiltered moments count it at the four exposures where it is on the grid
    assert xcor.reference(pairs, ob)[:, 0, 0].tolist() == [6.0, 6.0, 5.0, 6.0, 6.0]
    # the other columns do not know of it: the same values without it
    keep = np.arange(npix) != 4
    ob11 = xcor.Observed(xcor.segments([5, 6]), f[:, keep])
    assert np.array_equal(xcor.filter_reference(pairs[:, keep], ob11, F), got[:, keep])
    # a column with no value at all gives seven exact +0
    ob1 = xcor.Observed(xcor.segments([4, 1, 7]), f)
    z = xcor.reference_values(got, ob1)[:, 1]
    assert np.all(z == 0) and not np.any(np.signbit(z))


def test_an_all_zero_filter_changes_nothing():
    rng = np.random.default_rng(8)
    nexp, lens = 6, [3, 0, 70, 9]
    seg = xcor.segments(lens)
    npix = int(seg[-1])
    b = rng.uniform(0.5, 2.0, (nexp, npix))
    a = b * (1.0 + 0.2 * rng.standard_normal((nexp, npix)))
    b[:, 17] = 0.0                                                        # off the grid at every exposure
    pairs = np.stack([a, b], axis=-1)
    w = rng.uniform(0.5, 2.0, (nexp, npix))
    w[rng.random((nexp, npix)) < 0.1] = 0.0
    ob = xcor.Observed(seg, rng.standard_normal((nexp, npix)), w, rng.uniform(0.5, 1.5, npix))
    for ncomp in (1, 4):
        Z = xcor.Filter(np.zeros((len(lens), ncomp, nexp)), np.zeros((len(lens), nexp, ncomp)))
        val = xcor.filter_reference(pairs, ob, Z)
        with np.errstate(invalid="ignore", divide="ignore"):
            g = ob.gain[None, :] * (a / b)
        assert np.array_equal(val[:, b[0] > 0], g[:, b[0] > 0]) and np.isnan(val[:, 17]).all()
        assert np.array_equal(xcor.reference_values(val, ob), xcor.reference(pairs, ob))
        assert np.array_equal(xcor.abs_reference_values(val, ob), xcor.abs_reference(pairs, ob))


def test_library_exports_and_refuses_without_a_handle():
    path = build.lib_path("libtransit_hip.so")
    if not os.path.exists(path):
        build.build_hip()
    lib = C.CDLL(path)
    for name in ("trx_set_filter", "trx_run_filtered_moments", "trx_batch_set_filter", "trx_run_batch_filtered_moments"):
        assert hasattr(lib, name), name
    _abi.bind(lib, _abi.HIP_HEADER, "trx_")
    F = xcor.Filter(np.zeros((1, 1, 1)), np.zeros((1, 1, 1)))
    assert lib.trx_set_filter(None, C.byref(F.to_c())) == -1
    assert lib.trx_set_filter(None, None) == -1
    assert lib.trx_batch_set_filter(None, C.byref(F.to_c())) == -1
    mom, sh = np.zeros((1, 1, 7)), np.ones(1)
    assert lib.trx_run_filtered_moments(None, None, None, None, 1, sh.ctypes.data_as(_abi.c_double_p), None,
                                        mom.ctypes.data_as(_abi.c_double_p), None) == -1
    assert lib.trx_run_batch_filtered_moments(None, 0, None, None, 1, None, None) == -1
    lib.trx_abi_version.restype = C.c_int
    assert lib.trx_abi_version() == 5
    blob = open(path, "rb").read()
    assert b"k_pixel_filter" in blob and b"k_pixel_moments" in blob
