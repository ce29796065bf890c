"""The Kp-Vsys detection map on the device (trx_run_velocity_map / trx_run_batch_velocity_map, include/transit_hip.h):
trx_run_trail followed there by the statistic of every trail row added over the segments in order (per [nlag, nexp])
and by the map, per interpolated along every cell's velocity track and added over the exposures in order.

The case is xcor_checks': pixel_cases.make("eclipse", 20 000 lines, 6001 bins), the 800-pixel set, 7 exposures at
PHASE = linspace(-0.06, 0.06, 7), the lag grid -81 .. 81 km/s in steps of 3 (55 lags; 55 x 7 = 385 rows is no multiple of
the 4 rows of a block), and two observed sets: xcor_checks.observed() with the segments [1, 63, 64, 65, 200, 0, 7, 400] -- the
1-pixel and the empty segment are rows ccf and loglike_bl19 skip -- and the two-segment own-data set of
xcor_checks.end_to_end_map.  The map is Kp = 40, 70, 100, 130, 160, 190, 250 by Vsys = -12 .. 12 in steps of 6: with
sin(2 pi 0.06) = 0.36812 the Kp = 250 row is outside the lag grid everywhere (92.0 + |Vsys| > 81), the Kp = 190 row at
Vsys = +-12 only (81.9), everything else inside; the middle exposure has orbit = 0 and sits on lag nodes.  A second grid
of 13 x 11 = 143 cells is more than one block and ends in a ragged one.  More than one trip of a wave over the exposures
(k_velocity_map) and over the segments (k_trail_stat) -- 64, 65 and 130 of either -- is test_gpu_many_exposures.py's.

THE CONTRACT: map is bit for bit xcor.map_from_per of the per the same call returned; per is xcor.trail_statistic of
run_trail's trail within xcor.per_bound -- in the same bits for ccf and chi2, whose rows use only correctly rounded
operations, and to the accuracy of the device's log for loglike_bl19.  The tolerances are xcor.per_bound and
xcor.map_bound, derived in their docstrings."""
import ctypes as C

import numpy as np
import pytest

import pixel_cases as pc
import xcor_checks as xc
from transit_amd import _abi, broaden, pixels, xcor
from transit_amd.engine import Batch, Engine, EngineError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """(P, px, ob, trail): the eclipse case at 20 000 lines, the 800 pixels, the 8-segment observed set and run_trail's
    trail of it at the 55 lags"""
    P = pc.make(tmp_path_factory.mktemp("vmap"), "eclipse", nlines=20_000)
    px = xc.pixel_set(P)
    plain = Engine(P.static)
    scale = float(np.mean(plain.run(P.atm, P.opts)["spectrum"]))
    plain.close()
    ob = xc.observed(len(px), scale)
    E = xc.handle(P, px, ob)
    trail = E.run_trail(P.atm, P.opts, xc.LAGS)
    E.close()
    assert trail.shape == (55, 7, 8, 7) and xc.LAG_KMS.size == 55
    return P, px, ob, trail


def test_per_is_the_statistic_added_over_the_segments_in_order(case):
    P, px, ob, trail = case
    E = xc.handle(P, px, ob)
    # the 1-pixel and the empty segment are skipped by ccf and loglike_bl19; chi-square has a value for every row
    assert np.all(np.isnan(xcor.ccf(trail)[:, :, [0, 5]])) and np.all(np.isfinite(xcor.ccf(trail)[:, :, [1, 2, 3, 4, 6, 7]]))
    assert np.all(trail[:, :, 5] == 0) and np.all(trail[:, :, 0, 0] <= 1)
    for stat in xc.STATS:
        vm = xc.the_map(stat)
        m, per = E.run_velocity_map(P.atm, P.opts, vm, per=True)
        want = xc.check_per(per, trail, vm, "8 segments")
        if stat != "loglike_bl19":                             # (the expectation, printed above; the assertion is the bound)
            print("%s: per has numpy's bits: %s" % (stat, np.array_equal(per, want)))
        if stat == "ccf":                                       # skipped, not counted: six coefficients at the most
            assert np.all(np.abs(per) <= 6 * (1 + 1e-12))
    E.close()


@pytest.mark.parametrize("stat", xc.STATS)
def test_map_is_map_from_per_bit_for_bit(case, stat):
    P, px, ob, trail = case
    E = xc.handle(P, px, ob)
    pers = []
    for second in (False, True):
        for offset in (False, True):
            vm = xc.the_map(stat, second, offset)
            m, per = E.run_velocity_map(P.atm, P.opts, vm, per=True)
            assert m.shape == ((13, 11) if second else (7, 5))
            assert np.array_equal(m, xcor.map_from_per(per, vm), equal_nan=True), (stat, second, offset)
            if not second:
                assert np.array_equal(np.isnan(m), xc.OUTSIDE), (stat, offset)
            else:
                assert 0 < np.count_nonzero(np.isnan(m)) < m.size // 2
            pers.append(per)
            assert np.array_equal(E.run_velocity_map(P.atm, P.opts, vm), m, equal_nan=True)      # without per: the same map
    for per in pers[1:]:                                        # per does not depend on the cells
        assert np.array_equal(per, pers[0])
    E.close()


def test_own_data_map_peaks_at_the_injected_cell(case):
    P, px, _, _ = case
    E = Engine(P.static)
    E.set_pixels(px)
    seen = {}

    def trail_of(lags, ob):
        E.set_observed(ob)
        seen["ob"], seen["trail"] = ob, E.run_trail(P.atm, P.opts, lags)
        assert np.array_equal(lags, xc.LAGS)
        return seen["trail"]

    m5, cell = xc.end_to_end_map(px, lambda sh: E.run_pixels(P.atm, P.opts, sh), trail_of)
    assert cell == (2, 3) and seen["ob"].nseg == 2
    vm = xc.the_map("ccf")
    m = E.run_velocity_map(P.atm, P.opts, vm)                  # (the own-data set is still installed)
    vp = xc.VSYS[None, :, None] + xc.KP[:, None, None] * xc.ORBIT[None, None, :]
    old = xcor.velocity_map(seen["trail"], xc.LAG_KMS, vp, stat=xcor.ccf)
    bound = xcor.map_bound(seen["trail"], vm)
    assert np.array_equal(np.isnan(m), xc.OUTSIDE) and np.array_equal(np.isnan(old), xc.OUTSIDE)
    ratio = float(np.nanmax(np.abs(m - old) / bound))
    print("own data: worst |map - velocity_map(run_trail)| / map_bound %.4f; %d of 28 cells differ" % (ratio, np.count_nonzero(m[~xc.OUTSIDE] != old[~xc.OUTSIDE])))
    assert ratio <= 1.0
    assert np.array_equal(m[:5], m5) or float(np.max(np.abs(m[:5] - m5) / bound[:5])) <= 1.0
    peak = tuple(int(i) for i in np.unravel_index(np.nanargmax(m), m.shape))
    rest = np.where(np.arange(35).reshape(7, 5) == 2 * 5 + 3, np.nan, m)
    print("map (rows Kp, columns Vsys):\n%s\npeak %.4f at %s, at most %.4f elsewhere" % (np.array2string(m, precision=4), m[cell], peak, np.nanmax(rest)))
    assert peak == cell
    # numpy alone on the CPU, for the 5 x 5 cells of test_gpu_trail: 13.995 against at most 13.872
    assert 13.99 < m[cell] <= 14.0 and np.nanmax(rest[:5]) < 13.88
    E.close()


def test_cells_do_not_depend_on_the_rest_of_the_call_or_on_the_handles_history(case):
    P, px, ob, trail = case
    E = xc.handle(P, px, ob)
    for stat in xc.STATS:
        vm = xc.the_map(stat, offset=True)
        m = E.run_velocity_map(P.atm, P.opts, vm)
        rows, cols = [4, 1, 6, 3], [3, 0]
        sub = E.run_velocity_map(P.atm, P.opts, xc.the_map(stat, offset=True, kp=xc.KP[rows], vsys=xc.VSYS[cols]))
        assert np.array_equal(sub, m[np.ix_(rows, cols)], equal_nan=True), stat
        one = E.run_velocity_map(P.atm, P.opts, xc.the_map(stat, offset=True, kp=xc.KP[2:3], vsys=xc.VSYS[3:4]))
        assert one.shape == (1, 1) and one[0, 0] == m[2, 3]
        assert np.array_equal(E.run_velocity_map(P.atm, P.opts, vm), m, equal_nan=True)
    E.close()
    # fresh, hinted, resuming deeper, hinted again -- against a second handle's trail of the same atmosphere
    E, T = xc.handle(P, px, ob), xc.handle(P, px, ob)
    deep, keep = pc.thinner(P, 1e-3)
    vm = xc.the_map("loglike_bl19")
    seen = set()
    for k, atm in enumerate((P.atm, P.atm, deep, P.atm)):
        m, per, spec = E.run_velocity_map(atm, P.opts, vm, per=True, spectrum=True)
        tr, want_spec = T.run_trail(atm, P.opts, xc.LAGS, spectrum=True)
        assert np.array_equal(spec, want_spec), k
        assert np.array_equal(m, xcor.map_from_per(per, vm), equal_nan=True), k
        xc.check_per(per, tr, vm, "atmosphere %d" % k)
        seen.add(per.tobytes())
    assert len(seen) == 2
    E.close(); T.close()


def test_neighbours_on_the_handle_filter_and_broadening(case):
    P, px, ob, trail = case
    E = xc.handle(P, px, ob)
    vm = xc.the_map("ccf")
    before = (E.run_trail(P.atm, P.opts, xc.LAGS), E.run_moments(P.atm, P.opts, pc.SHIFTS), E.run_pixels(P.atm, P.opts, pc.SHIFTS))
    assert np.array_equal(before[0], trail)
    m, per = E.run_velocity_map(P.atm, P.opts, vm, per=True)
    after = (E.run_trail(P.atm, P.opts, xc.LAGS), E.run_moments(P.atm, P.opts, pc.SHIFTS), E.run_pixels(P.atm, P.opts, pc.SHIFTS))
    for a, b in zip(before, after):
        assert np.array_equal(a, b, equal_nan=True)
    # a filter takes no part
    E.set_filter(xcor.svd_filter(ob.data, ob.seg_first, 2))
    mf, pf = E.run_velocity_map(P.atm, P.opts, vm, per=True)
    assert np.array_equal(mf, m, equal_nan=True) and np.array_equal(pf, per)
    E.set_filter(None)
    # a broadening applies: the trail under it is run_trail's under it
    E.set_broadening(broaden.Rotation(4.0, 0.4))
    for stat in xc.STATS:
        vb = xc.the_map(stat)
        mb, pb = E.run_velocity_map(P.atm, P.opts, vb, per=True)
        broad = E.run_trail(P.atm, P.opts, xc.LAGS)
        assert np.array_equal(mb, xcor.map_from_per(pb, vb), equal_nan=True)
        xc.check_per(pb, broad, vb, "broadened")
        if stat == "ccf":
            assert np.all(pb != per)
    E.set_broadening(None)
    assert np.array_equal(E.run_velocity_map(P.atm, P.opts, vm), m, equal_nan=True)
    E.close()


def test_batch_maps_are_the_single_handle_maps(case):
    P, px, ob, _ = case
    K = 3
    atms, keep = pc.atmospheres(P, K)
    vm = xc.the_map("loglike_bl19", second=True, offset=True)
    one = xc.handle(P, px, ob)
    ref = [one.run_velocity_map(atms[j], P.opts, vm, per=True) for j in range(K)]
    one.close()
    assert len({r[1].tobytes() for r in ref}) == K
    B = Batch(P.static, ways=2)
    B.set_pixels(px)
    B.set_observed(ob)
    for rep in range(2):
        m, per = B.run_velocity_map(atms, P.opts, vm, per=True)
        assert m.shape == (K, 13, 11) and per.shape == (K, 55, 7)
        for j in range(K):
            assert np.array_equal(m[j], ref[j][0], equal_nan=True) and np.array_equal(per[j], ref[j][1]), (rep, j)
        assert np.array_equal(B.run_velocity_map(atms, P.opts, vm), m, equal_nan=True)
    B.close()


def test_one_lag(case):
    P, px, ob, _ = case
    E = xc.handle(P, px, ob)
    for stat in xc.STATS:
        vm = xc.the_map(stat, lag_kms=[6.0], kp=[100.0, 50.0], vsys=[6.0, 7.0], orbit=np.zeros(7))      # x = vsys: on the lag, or outside
        m, per = E.run_velocity_map(P.atm, P.opts, vm, per=True)
        assert per.shape == (1, 7) and m.shape == (2, 2)
        xc.check_per(per, E.run_trail(P.atm, P.opts, vm.lag), vm, "one lag")
        assert np.array_equal(m, xcor.map_from_per(per, vm), equal_nan=True)
        assert np.array_equal(np.isnan(m), [[False, True], [False, True]]) and m[0, 0] == m[1, 0]
    E.close()


def test_refusals(case):
    P, px, ob, _ = case
    dp = _abi.c_double_p
    E = Engine(P.static)
    lib = E._lib
    vm = xc.the_map("chi2", offset=True)
    with pytest.raises(EngineError) as ei:                     # no pixel set, no observed set
        E.run_velocity_map(P.atm, P.opts, vm)
    assert ei.value.code == -1 and "observed" in str(ei.value)
    E.set_pixels(px)
    E.set_observed(ob)
    before = E.run_velocity_map(P.atm, P.opts, vm, per=True)
    m, per = np.full((7, 5), -7.0), np.full((55, 7), -7.0)

    def run(c, to_map=m, to_per=per):
        rc = lib.trx_run_velocity_map(E._h, C.byref(P.atm), C.byref(P.opts), None, C.byref(c) if c is not None else None,
                                      to_map.ctypes.data_as(dp) if to_map is not None else None,
                                      to_per.ctypes.data_as(dp) if to_per is not None else None, None)
        assert np.all(m == -7.0) and np.all(per == -7.0)       # a refusal touches no output
        return rc, (lib.trx_last_error(E._h) or b"").decode()

    def changed(**fields):
        c = vm.to_c()
        for k, v in fields.items():
            setattr(c, k, v)
        return c

    def refused(c, text, **kw):
        rc, msg = run(c, **kw)
        assert rc == -1 and msg.startswith("trx_run_velocity_map: ") and text in msg, (text, rc, msg)

    refused(None, "vm is NULL")
    refused(vm.to_c(), "map is NULL", to_map=None)
    # what trx_run_trail refuses
    refused(changed(nlag=0), "nlag < 1")
    refused(changed(nlag=-2), "nlag < 1")
    refused(changed(lag=None), "lag is NULL")
    refused(changed(nlag=2 ** 26), "nlag * nexp * nseg above 2^31 - 1")      # (refused on the counts, before the lags are looked at)
    refused(changed(nlag=2 ** 30), "nlag * npix above what one pixel launch takes")
    for bad in (np.nan, np.inf, 0.0, -1.0):
        lag = vm.lag.copy()
        lag[1] = bad
        refused(xc.the_map("chi2", lag=lag).to_c(), "lag 1 must be finite and > 0")
    # the map's own
    refused(changed(stat=0), "unknown stat 0")
    refused(changed(stat=4), "unknown stat 4")
    refused(changed(nkp=0), "nkp < 1 or nvsys < 1")
    refused(changed(nvsys=-1), "nkp < 1 or nvsys < 1")
    refused(changed(nkp=2 ** 16, nvsys=2 ** 15), "nkp * nvsys above 2^31 - 1")
    for name in ("lag_kms", "kp", "vsys", "orbit"):
        refused(changed(**{name: None}), name + " is NULL")
    refused(changed(p0=np.nan), "p0 must be finite")
    refused(changed(p1=-np.inf), "p1 must be finite")
    for name, at in (("kp", 1), ("vsys", 4), ("orbit", 2), ("offset", 3)):
        for bad in (np.nan, np.inf):
            arr = np.array(getattr(vm, name), dtype=float)
            arr[at] = bad
            refused(xc.the_map("chi2", **{"offset": True, name: arr}).to_c(), "%s %d must be finite" % (name, at))
    for at, bad in ((0, np.nan), (54, np.inf), (2, xc.LAG_KMS[1]), (3, xc.LAG_KMS[1])):
        kms = xc.LAG_KMS.copy()
        kms[at] = bad
        refused(xc.the_map("chi2", offset=True, lag_kms=kms, lag=vm.lag).to_c(), "lag_kms %d must be finite and above" % at)
    # the handle is usable and the next run's bits are unchanged; per may be NULL
    alone = np.zeros((7, 5))
    assert lib.trx_run_velocity_map(E._h, C.byref(P.atm), C.byref(P.opts), None, C.byref(vm.to_c()), alone.ctypes.data_as(dp), None, None) == 0
    assert np.array_equal(alone, before[0], equal_nan=True)
    got = E.run_velocity_map(P.atm, P.opts, vm, per=True)
    assert np.array_equal(got[0], before[0], equal_nan=True) and np.array_equal(got[1], before[1])
    assert np.array_equal(E.run_velocity_map(P.atm, P.opts, vm), before[0], equal_nan=True)
    E.close()
    # a shard's partial pairs say nothing about the moments
    n = P.nwn
    try:
        P.set_shard(1000, 3000)
        S = Engine(P.static)
        S.set_pixels(pixels.Pixels([2510.0, 2520.0, 2530.0, 2540.0], [0.2, 0.3, 1.5, 0.4], 4.0))
        S.set_observed(xcor.Observed([0, 1, 4], np.ones((7, 4))))
        with pytest.raises(EngineError) as ei:
            S.run_velocity_map(P.atm, P.opts, vm)
        assert ei.value.code == -6 and "trx_gather_host" in str(ei.value)
        S.close()
    finally:
        P.set_shard(0, n)
    # the batch form
    B = Batch(P.static, ways=2)
    B.set_pixels(px)
    with pytest.raises(EngineError) as ei:                     # no observed set
        B.run_velocity_map([P.atm, P.atm], P.opts, vm)
    assert ei.value.code == -1 and "observed" in str(ei.value)
    B.set_observed(ob)
    ref = B.run_velocity_map([P.atm, P.atm], P.opts, vm, per=True)
    assert np.array_equal(ref[0][1], before[0], equal_nan=True) and np.array_equal(ref[1][0], before[1])
    maps, pers = np.full((2, 7, 5), -7.0), np.full((2, 55, 7), -7.0)
    arr = (_abi.TrxAtm * 2)(P.atm, P.atm)

    def batch(c, map_ptrs, per_ptrs):
        rc = lib.trx_run_batch_velocity_map(B._b, 2, arr, C.byref(P.opts), C.byref(c) if c is not None else None,
                                            (dp * 2)(*map_ptrs), (dp * 2)(*per_ptrs) if per_ptrs is not None else None)
        assert np.all(maps == -7.0) and np.all(pers == -7.0)
        return rc, (lib.trx_last_error(None) or b"").decode()

    mp, pp = [maps[j].ctypes.data_as(dp) for j in range(2)], [pers[j].ctypes.data_as(dp) for j in range(2)]
    assert batch(vm.to_c(), [mp[0], None], pp) == (-1, "trx_run_batch_velocity_map: map[1] is NULL")
    assert batch(vm.to_c(), mp, [pp[0], None]) == (-1, "trx_run_batch_velocity_map: per[1] is NULL")
    assert batch(None, mp, pp) == (-1, "trx_run_batch_velocity_map: vm is NULL")
    rc, msg = batch(changed(stat=9), mp, pp)
    assert rc == -1 and "unknown stat 9" in msg
    worse = vm.orbit.copy()
    worse[5] = np.nan
    with pytest.raises(EngineError) as ei:
        B.run_velocity_map([P.atm, P.atm], P.opts, xc.the_map("chi2", offset=True, orbit=worse))
    assert ei.value.code == -1 and "orbit 5 must be finite" in str(ei.value)
    again = B.run_velocity_map([P.atm, P.atm], P.opts, vm, per=True)
    assert np.array_equal(again[0], ref[0], equal_nan=True) and np.array_equal(again[1], ref[1])
    B.close()
