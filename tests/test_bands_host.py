"""The host-side band builders (transit_amd/bands.py) against independent integrals, and the GAUSS range rule of
trx_set_bands at its edges (no GPU)."""
import math

import numpy as np
import pytest

from transit_amd import _abi, bands


def grid(n=400, wn_i=2500.0, wn_d=0.5):
    return wn_i, wn_d, n, wn_i + np.arange(n) * wn_d


def box_integral(wn, d, S, lo, hi):
    """exact integral over [lo, hi] of the step function S_i on the cells [wn_i - d/2, wn_i + d/2], cell by cell"""
    tot = 0.0
    for x, s in zip(wn, S):
        a, b = max(x - d / 2, lo), min(x + d / 2, hi)
        if b > a:
            tot += (b - a) * s
    return tot


@pytest.mark.parametrize("lo,hi", [(2510.3, 2540.05), (2499.0, 2500.1), (2520.25, 2520.75), (2600.0, 2800.0),
                                   (2510.0, 2510.2)])
def test_tophat_is_the_box_integral(lo, hi):
    wn_i, wn_d, n, wn = grid()
    S = 1.0 + np.random.default_rng(1).random(n)
    b = bands.tophat(wn, lo, hi)
    assert b.kind == _abi.BAND_WEIGHTS and b.first >= 0 and b.first + b.weights.size <= n
    assert np.all(b.weights > 0) and np.all(b.weights <= 1)
    i = np.arange(b.first, b.first + b.weights.size)
    cover = min(hi, wn[-1] + wn_d / 2) - max(lo, wn[0] - wn_d / 2)
    assert math.fsum(b.weights) * wn_d == pytest.approx(cover, rel=1e-13)
    got = math.fsum(b.weights * S[i]) * wn_d
    assert got == pytest.approx(box_integral(wn, wn_d, S, lo, hi), rel=1e-13)


def test_tophats_tiling_the_grid_weigh_every_bin_once():
    wn_i, wn_d, n, wn = grid()
    edges = np.linspace(wn[0] - wn_d / 2, wn[-1] + wn_d / 2, 13)
    tot = np.zeros(n)
    for k in range(12):
        b = bands.tophat(wn, edges[k], edges[k + 1])
        tot[b.first:b.first + b.weights.size] += b.weights
    assert np.allclose(tot, 1.0, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        bands.tophat(wn, 100.0, 200.0)


def test_filter_curve_is_the_trapezoid_ratio():
    wn_i, wn_d, n, wn = grid()
    rng = np.random.default_rng(2)
    S = 1.0 + rng.random(n)
    fw = np.sort(rng.uniform(2530.0, 2610.0, 41))
    ft = np.exp(-((fw - 2570.0) / 20.0) ** 2)
    b = bands.filter_curve(wn, fw[::-1], ft[::-1])      # (any order of the filter's samples)
    inside = (wn >= fw[0]) & (wn <= fw[-1])
    x = wn[inside]
    assert b.first == np.flatnonzero(inside)[0] and b.weights.size == x.size
    f = np.interp(x, fw, ft)
    want = np.trapezoid(f * S[inside], x) / np.trapezoid(f, x)
    i = np.arange(b.first, b.first + b.weights.size)
    got = math.fsum(b.weights * S[i]) / math.fsum(b.weights)
    assert got == pytest.approx(want, rel=1e-13)
    assert math.fsum(b.weights) == pytest.approx(np.trapezoid(f, x), rel=1e-13)
    with pytest.raises(ValueError):
        bands.filter_curve(wn, [2530.1, 2530.2], [1.0, 1.0])     # fewer than two grid points inside


def members(wn_i, wn_d, n, c, fwhm, cut):
    """bins i with (c - cut sigma - wn_i)/wn_d <= i <= (c + cut sigma - wn_i)/wn_d, one by one"""
    sigma = fwhm / bands.FWHM_PER_SIGMA
    a = (c - cut * sigma - wn_i) / wn_d
    z = (c + cut * sigma - wn_i) / wn_d
    return [i for i in range(n) if a <= i <= z]


def test_gauss_range_rule():
    wn_i, wn_d, n, wn = grid()
    rng = np.random.default_rng(3)
    cases = [(float(c), float(f), float(k)) for c, f, k in zip(rng.uniform(2490, 2710, 200), rng.uniform(0.01, 5, 200),
                                                                 rng.uniform(0.5, 6, 200))]
    # edges on grid points: sigma = 0.5 and 0.25 exactly, cut sigma a whole number of bins
    for fwhm, cut in ((0.5 * bands.FWHM_PER_SIGMA, 4.0), (0.25 * bands.FWHM_PER_SIGMA, 2.0)):
        assert fwhm / bands.FWHM_PER_SIGMA in (0.5, 0.25)
        cases += [(float(wn[k]), fwhm, cut) for k in (0, 1, 3, 200, n - 4, n - 2, n - 1)]
    cases += [(wn[0] - 1000.0, 1.0, 4.0), (wn[-1] + 1000.0, 1.0, 4.0), (wn[0] - 10.0, 100.0, 4.0)]
    for c, f, k in cases:
        a, z = bands.gauss_range(wn_i, wn_d, n, c, f, k)
        m = members(wn_i, wn_d, n, c, f, k)
        assert 0 <= a <= z <= n
        assert list(range(a, z)) == m, (c, f, k)
    # the exact edges are in: 4 sigmas = 4 bins either side
    a, z = bands.gauss_range(wn_i, wn_d, n, float(wn[200]), 0.5 * bands.FWHM_PER_SIGMA, 4.0)
    assert (a, z) == (196, 205)
    a, z = bands.gauss_range(wn_i, wn_d, n, float(wn[1]), 0.5 * bands.FWHM_PER_SIGMA, 4.0)
    assert (a, z) == (0, 6)
    assert bands.gauss_range(wn_i, wn_d, n, wn[0] - 1000.0, 1.0, 4.0) == (0, 0)
    assert bands.gauss_range(wn_i, wn_d, n, wn[-1] + 1000.0, 1.0, 4.0) == (n, n)


def test_gauss_builders():
    b = bands.gauss(2600.0, 1.5)
    assert (b.kind, b.centre, b.fwhm, b.cut) == (_abi.BAND_GAUSS, 2600.0, 1.5, 4.0)
    bs = bands.resolving_power([2000.0, 3000.0], 3000.0, cut=3.0)
    assert [(x.centre, x.fwhm, x.cut) for x in bs] == [(2000.0, 2000.0 / 3000.0, 3.0), (3000.0, 1.0, 3.0)]


def test_struct_and_combine():
    bs = [bands.weights(5, [1.0, 2.0]), bands.gauss(2600.0, 1.5, 3.0)]
    arr = bands.to_c(bs)
    assert _abi.C.sizeof(_abi.TrxBand) == 56
    assert (arr[0].kind, arr[0].first, arr[0].n, arr[0].weights[1]) == (0, 5, 2, 2.0)
    assert (arr[1].kind, arr[1].n, arr[1].centre, arr[1].fwhm, arr[1].cut) == (1, 0, 2600.0, 1.5, 3.0)
    parts = [np.array([[1e16, 1.0]]), np.array([[1.0, 2.0]]), np.array([[-1e16, 3.0]])]
    assert bands.combine(parts).tolist() == [[((1e16 + 1.0) - 1e16), 6.0]]        # in the order given
    assert bands.value(np.array([[3.0, 2.0], [1.0, 4.0]])).tolist() == [1.5, 0.25]
