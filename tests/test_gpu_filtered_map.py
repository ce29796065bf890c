"""The Kp-Vsys detection map with the detrending filter applied to every cell's own model matrix, on the device
(trx_run_filtered_map / trx_run_batch_filtered_map, include/transit_hip.h).

The case is xcor_checks': pixel_cases.make("eclipse", 20 000 lines, 6001 bins), the 800 pixels, 7 exposures, the
segments [1, 63, 64, 65, 200, 0, 7, 400], the 55 lags -81 .. 81 km/s, the 7 x 5 map with its seven outside cells and the
13 x 11 map -- 143 cells, three chunks of _abi.CELLMAP_CHUNK = 64 cells with a ragged last one (second_axes enlarges the grid
should the cap ever grow).  The filter is xcor.svd_filter(ob.data, ob.seg_first, 3).  One pixel (PIXEL, of segment 2) is moved
to the grid's upper edge, so that its window is on the grid for the lags up to +30 km/s only: its column is live in the cells
whose whole track stays below that, dead in the others.

THE CONTRACT (test 1): a cell's value is points 5 of the definition -- xcor.cell_value -- applied to the moments
run_filtered_moments returns on the same handle at the shifts LAGS[lag_index[cell]], within xcor.cell_bound (derived in its
docstring), and in the same bits for ccf and chi2 in practice (printed).

AGAINST NUMPY ALONE (test 2): the map against xcor.filtered_map_reference of run_pixels' pairs at the lags.  The tolerance is
the plain filter's tolerance of the VALUES carried through the moments and the statistic, derived in the docstring of
xcor_checks.row_bounds; nothing in it is measured, and the relative changes it rests on are asserted below 1e-3."""
import ctypes as C

import numpy as np
import pytest

import pixel_cases as pc
import xcor_checks as xc
from transit_amd import _abi, bands, broaden, pixels, xcor
from transit_amd.engine import Batch, Engine, EngineError

pytestmark = pytest.mark.gpu

STATS = xc.STATS
LAG_KMS, LAGS = xc.LAG_KMS, xc.LAGS
OUTSIDE = xc.OUTSIDE


def handle(case, filt=True):
    E = xc.handle(case.P, case.px, case.ob)
    if filt:
        E.set_filter(case.F)
    return E


class Case:
    """the problem, the pixel set with PIXEL at the grid's edge, the observed set, the filter, the pairs at the 55 lags, and
    -- made once, on first use, shared by the tests -- the filtered moments of every distinct lag row a map's cells take"""

    def __init__(self, P, px, ob, F):
        self.P, self.px, self.ob, self.F = P, px, ob, F
        E = handle(self)
        self.pairs = E.run_pixels(P.atm, P.opts, LAGS)
        E.close()
        self.moms = {}

    def moments(self, E, idx, key="plain"):
        """run_filtered_moments on E at LAGS[idx], once per distinct idx (and per key: what is installed on E)"""
        k = (key, np.asarray(idx, dtype=np.int64).tobytes())
        if k not in self.moms:
            self.moms[k] = E.run_filtered_moments(self.P.atm, self.P.opts, LAGS[idx])
        return self.moms[k]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    P = pc.make(tmp_path_factory.mktemp("fmap"), "eclipse", nlines=20_000)
    px = xc.pixel_set(P)
    # PIXEL's window [c - h, c + h] / lag leaves the grid (its last point: wn_i + (n - 1) wn_d) between the lags of
    # +30 and +33 km/s: its lower edge, at the lag of +31.5 km/s, sits half a bin above the last grid point
    wn_i, wn_d, n = float(P.static.wn_i), float(P.static.wn_d), int(P.static.nwn)
    half = px.cut * px.fwhm[xc.PIXEL] / bands.FWHM_PER_SIGMA
    px.centre[xc.PIXEL] = (wn_i + (n - 0.5) * wn_d) * pixels.shift(xc.LIVE_UP_TO + 1.5) + half
    plain = Engine(P.static)
    scale = float(np.mean(plain.run(P.atm, P.opts)["spectrum"]))
    plain.close()
    ob = xc.observed(len(px), scale)
    assert ob.seg_first[2] <= xc.PIXEL < ob.seg_first[3]
    c = Case(P, px, ob, xcor.svd_filter(ob.data, ob.seg_first, 3))
    assert c.pairs.shape == (55, 800, 2)
    assert np.array_equal(c.pairs[:, xc.PIXEL, 1] > 0, LAG_KMS <= xc.LIVE_UP_TO)
    return c


@pytest.mark.parametrize("stat", STATS)
def test_a_cell_is_the_filtered_moments_at_its_nearest_lags(case, stat):
    E = handle(case)
    for second in (False, True):
        for offset in ((False, True) if not second else (True,)):
            vm = xc.the_filtered_map(stat, second, offset)
            m, idx = E.run_filtered_map(case.P.atm, case.P.opts, vm, lag_index=True)
            want_idx = xcor.nearest_lags(vm)
            assert idx.dtype == np.int32 and idx.shape == want_idx.shape == (vm.nkp, vm.nvsys, 7)
            assert np.array_equal(idx, want_idx)
            outside = np.any(want_idx < 0, axis=-1)
            assert np.array_equal(np.isnan(m), outside)
            if not second:
                assert np.array_equal(outside, OUTSIDE)
            else:
                assert m.size > 2 * xc.CHUNK and m.size % xc.CHUNK != 0 and 0 < np.count_nonzero(outside) < m.size // 2
            # the moved pixel's column is live in some inside cells and dead in others
            live = np.array([[np.all(case.pairs[np.maximum(idx[i, j], 0), xc.PIXEL, 1] > 0) for j in range(vm.nvsys)] for i in range(vm.nkp)])
            assert np.any(live & ~outside) and np.any(~live & ~outside)
            differ = xc.check_contract(case, E, vm, m, idx, what="%d cells%s" % (m.size, ", offset" if offset else ""))
            if stat != "loglike_bl19":                             # (the expectation, printed; the assertion is the bound)
                print("%s: the map has the bits of the host's points 5: %s" % (stat, differ == 0))
    E.close()


@pytest.mark.parametrize("stat", STATS)
def test_the_map_is_the_definition_in_numpy(case, stat):
    E = handle(case)
    vm = xc.the_filtered_map(stat, offset=True)
    m, idx = E.run_filtered_map(case.P.atm, case.P.opts, vm, lag_index=True)
    E.close()
    ref = xcor.filtered_map_reference(case.pairs, case.ob, case.F, vm)
    assert np.array_equal(np.isnan(m), OUTSIDE) and np.array_equal(np.isnan(ref), OUTSIDE)
    worst = 0.0
    for i, j in np.argwhere(~OUTSIDE):
        mom, D = xc.moment_differences(case, case.pairs[idx[i, j]])
        assert xcor.cell_value(mom, vm) == ref[i, j]
        rows, small = xc.row_bounds(mom, D, vm)
        assert small < 1e-3, (stat, i, j, small)
        tol = 2.0 * float(np.sum(rows)) + xcor.cell_bound(mom, vm)
        assert tol > 0 and abs(m[i, j] - ref[i, j]) <= tol, (stat, i, j, m[i, j], ref[i, j], tol)
        worst = max(worst, abs(m[i, j] - ref[i, j]) / tol)
    print("%s: worst |map - filtered_map_reference| / tolerance %.3e over the %d inside cells" % (stat, worst, np.count_nonzero(~OUTSIDE)))


def test_cells_do_not_depend_on_the_rest_of_the_call_or_on_the_handles_history(case):
    P = case.P
    E = handle(case)
    plain = Engine(P.static)
    spec_ref = plain.run(P.atm, P.opts)["spectrum"]
    plain.close()
    for stat in STATS:
        vm = xc.the_filtered_map(stat, offset=True)
        m = E.run_filtered_map(P.atm, P.opts, vm)
        # one cell alone: another launch, the first place of the only chunk
        for i, j in ((2, 3), (5, 2), (0, 0)):
            one = E.run_filtered_map(P.atm, P.opts, xc.the_filtered_map(stat, offset=True, kp=xc.KP[i:i + 1], vsys=xc.VSYS[j:j + 1]))
            assert one.shape == (1, 1) and one[0, 0] == m[i, j], (stat, i, j)
        # the axes reversed: every cell at another place of its chunk -- and, in the 143-cell map, in another chunk
        rev = E.run_filtered_map(P.atm, P.opts, xc.the_filtered_map(stat, offset=True, kp=xc.KP[::-1], vsys=xc.VSYS[::-1]))
        assert np.array_equal(rev[::-1, ::-1], m, equal_nan=True), stat
        vm2 = xc.the_filtered_map(stat, second=True)
        m2 = E.run_filtered_map(P.atm, P.opts, vm2)
        rev2 = E.run_filtered_map(P.atm, P.opts, xc.the_filtered_map(stat, second=True, kp=xc.FMAP_KP2[::-1], vsys=xc.FMAP_VSYS2[::-1]))
        assert np.array_equal(rev2[::-1, ::-1], m2, equal_nan=True), stat
        # with and without the table, with and without the spectrum
        a, idx = E.run_filtered_map(P.atm, P.opts, vm, lag_index=True)
        b, spec = E.run_filtered_map(P.atm, P.opts, vm, spectrum=True)
        c, idx2, spec2 = E.run_filtered_map(P.atm, P.opts, vm, lag_index=True, spectrum=True)
        for x in (a, b, c):
            assert np.array_equal(x, m, equal_nan=True), stat
        assert np.array_equal(idx, idx2) and np.array_equal(spec, spec_ref) and np.array_equal(spec2, spec_ref)
    E.close()
    # fresh, hinted, resuming deeper, hinted again -- the moments from a second handle at the same atmosphere
    E, T = handle(case), handle(case)
    deep, keep = pc.thinner(P, 1e-3)
    vm = xc.the_filtered_map("loglike_bl19", offset=True)
    seen = set()
    for k, atm in enumerate((P.atm, P.atm, deep, P.atm)):
        m, idx, spec = E.run_filtered_map(atm, P.opts, vm, lag_index=True, spectrum=True)
        assert np.array_equal(idx, xcor.nearest_lags(vm)) and np.array_equal(np.isnan(m), OUTSIDE), k
        for i, j in ((0, 0), (2, 3), (4, 4), (5, 1)):
            mom, want_spec = T.run_filtered_moments(atm, P.opts, LAGS[idx[i, j]], spectrum=True)
            assert np.array_equal(spec, want_spec), k
            assert abs(m[i, j] - xcor.cell_value(mom, vm)) <= xcor.cell_bound(mom, vm), (k, i, j)
        seen.add(m.tobytes())
    assert len(seen) == 2
    E.close(); T.close()


def test_with_a_highpass_and_a_broadening_installed(case):
    P = case.P
    E = handle(case)
    plain = {stat: E.run_filtered_map(P.atm, P.opts, xc.the_filtered_map(stat)) for stat in STATS}
    E.set_highpass(xcor.gaussian_highpass(6.0))
    E.set_broadening(broaden.Rotation(4.0, 0.4))
    for stat in STATS:
        vm = xc.the_filtered_map(stat)
        m, idx = E.run_filtered_map(P.atm, P.opts, vm, lag_index=True)
        assert np.array_equal(idx, xcor.nearest_lags(vm)) and np.array_equal(np.isnan(m), OUTSIDE)
        assert np.all(m[~OUTSIDE] != plain[stat][~OUTSIDE])
        xc.check_contract(case, E, vm, m, idx, key="highpass and broadening", what="high-pass and broadening")
    E.set_highpass(None)
    E.set_broadening(None)
    for stat in STATS:
        assert np.array_equal(E.run_filtered_map(P.atm, P.opts, xc.the_filtered_map(stat)), plain[stat], equal_nan=True)
    E.close()


def test_the_trail_and_the_velocity_map_are_unchanged(case):
    P = case.P
    E = handle(case, filt=False)
    vm = xc.the_filtered_map("ccf", offset=True)

    def neighbours():
        return (E.run_trail(P.atm, P.opts, LAGS),) + E.run_velocity_map(P.atm, P.opts, vm, per=True)

    def same(a, b):
        return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))

    without = neighbours()
    E.set_filter(case.F)
    with_filter = neighbours()
    assert same(without, with_filter)
    m = E.run_filtered_map(P.atm, P.opts, vm)
    assert same(neighbours(), without)
    # the trail the device keeps is the last trail run's: a filtered map writes none, and the next map run makes its own
    assert np.array_equal(E.run_filtered_map(P.atm, P.opts, vm), m, equal_nan=True)
    E.set_filter(None)
    assert same(neighbours(), without)
    E.close()


def test_an_all_zero_filter_on_lag_nodes_is_the_velocity_map(case):
    """orbit = 0 and Vsys on lag nodes: every track sits on a node, t = 0, and the velocity map takes per[k] as it stands"""
    P = case.P
    E = handle(case, filt=False)
    E.set_filter(xcor.Filter(np.zeros((8, 1, 7)), np.zeros((8, 7, 1))))
    nodes = LAG_KMS[[0, 10, 27, 38, 53]]
    for stat in STATS:
        vm = xc.the_filtered_map(stat, kp=[100.0, 50.0], vsys=nodes, orbit=np.zeros(7))
        assert np.array_equal(xcor.nearest_lags(vm)[0, :, 3], [0, 10, 27, 38, 53])
        m, want = E.run_filtered_map(P.atm, P.opts, vm), E.run_velocity_map(P.atm, P.opts, vm)
        assert np.all(np.isfinite(m)) and np.array_equal(m[0], m[1])
        if stat == "loglike_bl19":                              # (both from the device's log: printed, not asserted)
            print("loglike_bl19: the bits of the velocity map: %s" % np.array_equal(m, want))
        else:
            assert np.array_equal(m, want), stat
    E.close()


def test_refusals_and_the_batch_form(case):
    P, px, ob = case.P, case.px, case.ob
    dp = _abi.c_double_p
    E = Engine(P.static)
    lib = E._lib
    vm = xc.the_filtered_map("chi2", offset=True)
    with pytest.raises(EngineError) as ei:                     # no pixel set, no observed set
        E.run_filtered_map(P.atm, P.opts, vm)
    assert ei.value.code == -1 and "trx_run_filtered_map: no observed set installed (trx_set_observed)" in str(ei.value)
    E.set_pixels(px)
    E.set_observed(ob)
    with pytest.raises(EngineError) as ei:
        E.run_filtered_map(P.atm, P.opts, vm)
    assert ei.value.code == -1 and "trx_run_filtered_map: no filter installed (trx_set_filter)" in str(ei.value)
    E.set_filter(case.F)
    before = E.run_filtered_map(P.atm, P.opts, vm, lag_index=True)
    m, idx = np.full((7, 5), -7.0), np.full((7, 5, 7), -7, dtype=np.int32)

    def run(c, to_map=m):
        rc = lib.trx_run_filtered_map(E._h, C.byref(P.atm), C.byref(P.opts), None, C.byref(c) if c is not None else None,
                                      to_map.ctypes.data_as(dp) if to_map is not None else None, idx.ctypes.data_as(_abi.c_int32_p), None)
        assert np.all(m == -7.0) and np.all(idx == -7)         # a refusal touches no output
        return rc, (lib.trx_last_error(E._h) or b"").decode()

    def changed(**fields):
        c = vm.to_c()
        for k, v in fields.items():
            setattr(c, k, v)
        return c

    def refused(c, text, **kw):
        rc, msg = run(c, **kw)
        assert rc == -1 and msg == "trx_run_filtered_map: " + text, (text, rc, msg)

    # a map run's refusals, under this call's name
    refused(None, "vm is NULL")
    refused(vm.to_c(), "map is NULL", to_map=None)
    refused(changed(nlag=0), "nlag < 1")
    refused(changed(lag=None), "lag is NULL")
    refused(changed(nlag=2 ** 26), "nlag * nexp * nseg above 2^31 - 1")
    refused(changed(nlag=2 ** 30), "nlag * npix above what one pixel launch takes")
    lag = vm.lag.copy()
    lag[1] = np.nan
    refused(xc.the_filtered_map("chi2", lag=lag).to_c(), "lag 1 must be finite and > 0")
    refused(changed(stat=4), "unknown stat 4")
    refused(changed(nkp=0), "nkp < 1 or nvsys < 1")
    refused(changed(nkp=2 ** 16, nvsys=2 ** 15), "nkp * nvsys above 2^31 - 1")
    for name in ("lag_kms", "kp", "vsys", "orbit"):
        refused(changed(**{name: None}), name + " is NULL")
    refused(changed(p0=np.nan), "p0 must be finite")
    worse = vm.orbit.copy()
    worse[2] = np.inf
    refused(xc.the_filtered_map("chi2", offset=True, orbit=worse).to_c(), "orbit 2 must be finite")
    kms = LAG_KMS.copy()
    kms[3] = kms[2]
    refused(xc.the_filtered_map("chi2", offset=True, lag_kms=kms, lag=vm.lag).to_c(), "lag_kms 3 must be finite and above the one before it (strictly increasing)")
    # its own: the index table's size (2^15 x 2^14 cells pass the map's limit; seven exposures of them do not)
    long_kp, long_vsys = np.full(2 ** 15, 100.0), np.zeros(2 ** 14)
    refused(changed(nkp=2 ** 15, nvsys=2 ** 14, kp=long_kp.ctypes.data_as(dp), vsys=long_vsys.ctypes.data_as(dp)), "nkp * nvsys * nexp above 2^31 - 1")
    # the handle is usable and the next run's bits are unchanged; lag_index may be NULL
    alone = np.zeros((7, 5))
    assert lib.trx_run_filtered_map(E._h, C.byref(P.atm), C.byref(P.opts), None, C.byref(vm.to_c()), alone.ctypes.data_as(dp), None, None) == 0
    assert np.array_equal(alone, before[0], equal_nan=True)
    got = E.run_filtered_map(P.atm, P.opts, vm, lag_index=True)
    assert np.array_equal(got[0], before[0], equal_nan=True) and np.array_equal(got[1], before[1])
    # a shard's partial pairs say nothing about the live columns or the moments
    n = P.nwn
    try:
        P.set_shard(1000, 3000)
        S = Engine(P.static)
        S.set_pixels(pixels.Pixels([2510.0, 2520.0, 2530.0, 2540.0], [0.2, 0.3, 1.5, 0.4], 4.0))
        S.set_observed(xcor.Observed([0, 1, 4], np.ones((7, 4))))
        with pytest.raises(EngineError) as ei:
            S.run_filtered_map(P.atm, P.opts, vm)
        assert ei.value.code == -6 and "trx_run_filtered_map: this handle's shard is not the whole grid" in str(ei.value)
        S.close()
    finally:
        P.set_shard(0, n)
    # the batch form: three atmospheres on two ways, a broadening each
    K = 3
    atms, keep = pc.atmospheres(P, K)
    rot = [broaden.Rotation(4.0, 0.4), broaden.Rotation(2.5, 0.1), broaden.Rotation(6.0, 0.8)]
    vm2 = xc.the_filtered_map("loglike_bl19", second=True, offset=True)
    ref = []
    for j in range(K):
        E.set_broadening(rot[j])
        ref.append(E.run_filtered_map(atms[j], P.opts, vm2))
    E.close()
    assert len({r.tobytes() for r in ref}) == K
    B = Batch(P.static, ways=2)
    B.set_pixels(px)
    with pytest.raises(EngineError) as ei:                     # no observed set
        B.run_filtered_map(atms, P.opts, vm2)
    assert ei.value.code == -1 and "trx_run_batch_filtered_map: no observed set installed (trx_batch_set_observed)" in str(ei.value)
    B.set_observed(ob)
    with pytest.raises(EngineError) as ei:                     # no filter
        B.run_filtered_map(atms, P.opts, vm2)
    assert ei.value.code == -1 and "trx_run_batch_filtered_map: no filter installed (trx_batch_set_filter)" in str(ei.value)
    B.set_filter(case.F)
    B.set_broadening(rot)
    for rep in range(2):
        maps = B.run_filtered_map(atms, P.opts, vm2)
        assert maps.shape == (K, vm2.nkp, vm2.nvsys)
        for j in range(K):
            assert np.array_equal(maps[j], ref[j], equal_nan=True), (rep, j)
    with pytest.raises(EngineError) as ei:                     # two broadenings for three atmospheres
        B.set_broadening(rot[:2])
        B.run_filtered_map(atms, P.opts, vm2)
    assert ei.value.code == -1 and "2 broadenings installed" in str(ei.value)
    B.set_broadening(rot)
    out = np.full((K, vm2.nkp, vm2.nvsys), -7.0)
    arr = (_abi.TrxAtm * K)(*atms)

    def batch(c, ptrs):
        rc = lib.trx_run_batch_filtered_map(B._b, K, arr, C.byref(P.opts), C.byref(c) if c is not None else None, (dp * K)(*ptrs))
        assert np.all(out == -7.0)
        return rc, (lib.trx_last_error(None) or b"").decode()

    ptrs = [out[j].ctypes.data_as(dp) for j in range(K)]
    assert batch(vm2.to_c(), [ptrs[0], None, ptrs[2]]) == (-1, "trx_run_batch_filtered_map: map[1] is NULL")
    assert batch(None, ptrs) == (-1, "trx_run_batch_filtered_map: vm is NULL")
    c = vm2.to_c()
    c.stat = 9
    assert batch(c, ptrs) == (-1, "trx_run_batch_filtered_map: unknown stat 9")
    assert np.array_equal(B.run_filtered_map(atms, P.opts, vm2), maps, equal_nan=True)
    B.close()
