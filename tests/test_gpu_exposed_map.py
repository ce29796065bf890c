"""The detrended Kp-Vsys map under the exposure table, on the device (trx_run_exposed_map / trx_run_batch_exposed_map,
include/transit_hip.h).

The case is xcor_checks': pixel_cases.make("eclipse", 20 000 lines, 6001 bins), the 800 pixels, 7 exposures, the segments
[1, 63, 64, 65, 200, 0, 7, 400], the 55 lags -81 .. 81 km/s, the 7 x 5 map with its seven outside cells, the 13 x 11 map of
three chunks with a ragged last one, the filter xcor.svd_filter(ob.data, ob.seg_first, 3) and the pixel (PIXEL) at the grid's
upper edge whose column is live in some cells only.  On top of it the table xcor_checks.SCALE and SMEAR: scales with 1, 0 and a
negative value, smears that mix exact 0 with half-widths up to 1.3e-5 (7.8 km/s across the exposure).

THE CONTRACT (test 1): a cell's value is xcor.cell_value of the moments run_filtered_moments returns on the same handle,
table installed, at the shifts LAGS[lag_index[cell]], within xcor.cell_bound -- and in the same bits for ccf and chi2 in
practice (printed).

AGAINST NUMPY ALONE (test 3): the map against xcor.exposed_map_reference of pairs_lv, run_exposed's pairs at a constant shift
per lag.  The tolerance is the one derived in xcor_checks.row_bounds' docstring, applied to each cell's own rows
pairs_lv[lag_index[cell][v]][v]; nothing in it is measured, and the relative changes it rests on are asserted below 1e-3."""
import ctypes as C

import numpy as np
import pytest

import pixel_cases as pc
import wfilter_cases as wc
import xcor_checks as xc
from bits import same_bits
from transit_amd import _abi, bands, broaden, pixels, xcor
from transit_amd.engine import Batch, Engine, EngineError
from transit_amd.exposures import Exposures

pytestmark = pytest.mark.gpu

STATS = xc.STATS
LAG_KMS, LAGS = xc.LAG_KMS, xc.LAGS
OUTSIDE = xc.OUTSIDE
KP2, VSYS2 = xc.FMAP_KP2, xc.FMAP_VSYS2
CHUNK = xc.CHUNK
PIXEL, LIVE_UP_TO = xc.PIXEL, xc.LIVE_UP_TO
SCALE, SMEAR = xc.SCALE, xc.SMEAR
the_map = xc.the_filtered_map


def table():
    return Exposures(SCALE.copy(), SMEAR.copy())


def handle(case, filt=True, ex=True):
    E = xc.handle(case.P, case.px, case.ob)
    if filt:
        E.set_filter(case.F)
    if ex is not None and ex is not False:
        E.set_exposures(table() if ex is True else ex)
    return E


class Case:
    """the problem, the pixel set with PIXEL at the grid's edge, the observed set, the filter, run_exposed's pairs of every
    exposure at every lag under the table, and -- made once, on first use, shared by the tests -- the filtered moments of
    every distinct lag row a map's cells take"""

    def __init__(self, P, px, ob, F):
        self.P, self.px, self.ob, self.F = P, px, ob, F
        E = handle(self)
        self.pairs_lv = np.stack([E.run_exposed(P.atm, P.opts, np.full(ob.nexp, s)) for s in LAGS])
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
    P = pc.make(tmp_path_factory.mktemp("expmap"), "eclipse", nlines=20_000)
    px = xc.pixel_set(P)
    # (xcor_checks.PIXEL: its window leaves the grid between the lags of +30 and +33 km/s)
    wn_i, wn_d, n = float(P.static.wn_i), float(P.static.wn_d), int(P.static.nwn)
    half = px.cut * px.fwhm[PIXEL] / bands.FWHM_PER_SIGMA
    px.centre[PIXEL] = (wn_i + (n - 0.5) * wn_d) * pixels.shift(LIVE_UP_TO + 1.5) + half
    plain = Engine(P.static)
    scale = float(np.mean(plain.run(P.atm, P.opts)["spectrum"]))
    plain.close()
    ob = xc.observed(len(px), scale)
    assert ob.seg_first[2] <= PIXEL < ob.seg_first[3] and (ob.nexp, ob.nseg) == (7, 8)
    assert SCALE.size == SMEAR.size == 7 and 0.0 in SCALE and 1.0 in SCALE and SCALE.min() < 0 and 0.0 in SMEAR and SMEAR.max() > 1e-5
    c = Case(P, px, ob, xcor.svd_filter(ob.data, ob.seg_first, 3))
    assert c.pairs_lv.shape == (55, 7, 800, 2)
    # (an exposure without smear loses the pixel where the plain rows do; a smeared window is wider and keeps a bin for a
    # lag or two more; at the last lags it is gone at every exposure)
    assert SMEAR[0] == 0.0 and np.array_equal(c.pairs_lv[:, 0, PIXEL, 1] > 0, LAG_KMS <= LIVE_UP_TO)
    assert np.all(c.pairs_lv[LAG_KMS <= LIVE_UP_TO][:, :, PIXEL, 1] > 0) and np.all(c.pairs_lv[-10:, :, PIXEL, 1] == 0)
    return c


def run(E, case, vm, atm=None):
    """(map, lag_index, nrows), with what holds for every call asserted"""
    m, idx, R = E.run_exposed_map(atm if atm is not None else case.P.atm, case.P.opts, vm, lag_index=True, nrows=True)
    want_idx = xcor.nearest_lags(vm)
    assert idx.dtype == np.int32 and idx.shape == want_idx.shape == (vm.nkp, vm.nvsys, 7) and np.array_equal(idx, want_idx)
    assert np.array_equal(np.isnan(m), np.any(want_idx < 0, axis=-1))
    assert R == xcor.exposed_map_rows(vm)[3]
    return m, idx, R


@pytest.mark.parametrize("stat", STATS)
def test_a_cell_is_the_filtered_moments_under_the_table(case, stat):
    E = handle(case)
    for second in (False, True):
        for offset in ((False, True) if not second else (True,)):
            vm = the_map(stat, second, offset)
            m, idx, R = run(E, case, vm)
            outside = np.isnan(m)
            if not second:
                assert np.array_equal(outside, OUTSIDE)
            else:
                assert m.size > 2 * CHUNK and m.size % CHUNK != 0 and 0 < np.count_nonzero(outside) < m.size // 2
            # the rows are (lag, exposure) pairs: fewer than every lag at every exposure, more than one per exposure
            assert 7 < R < 7 * 55
            # the moved pixel's column is live in some inside cells and dead in others
            ve = np.arange(7)
            live = np.array([[np.all(case.pairs_lv[np.maximum(idx[i, j], 0), ve, PIXEL, 1] > 0) for j in range(vm.nvsys)] for i in range(vm.nkp)])
            assert np.any(live & ~outside) and np.any(~live & ~outside)
            # the table matters: no inside cell has the filtered map's value
            plain = E.run_filtered_map(case.P.atm, case.P.opts, vm)
            assert np.array_equal(np.isnan(plain), outside) and np.all(plain[~outside] != m[~outside])
            differ = xc.check_contract(case, E, vm, m, idx, key="table", what="%d cells, R = %d%s" % (m.size, R, ", offset" if offset else ""))
            if stat != "loglike_bl19":                             # (the expectation, printed; the assertion is the bound)
                print("%s: the map has the bits of the host's points 5: %s" % (stat, differ == 0))
    E.close()


def test_a_table_that_changes_nothing_gives_the_filtered_map(case):
    P = case.P
    E = handle(case, ex=None)
    want = {}
    for stat in STATS:
        for second in (False, True):
            want[stat, second] = E.run_filtered_map(P.atm, P.opts, the_map(stat, second, True), lag_index=True)
    for name, ex in (("scale 1, smear 0", Exposures(np.ones(7), np.zeros(7))), ("scale 1", Exposures(scale=np.ones(7))), ("smear 0", Exposures(smear=np.zeros(7)))):
        E.set_exposures(ex)
        for (stat, second), (wm, widx) in want.items():
            m, idx, R = run(E, case, the_map(stat, second, True))
            assert same_bits(m, wm) and np.array_equal(idx, widx), (name, stat, second)
    E.close()


@pytest.mark.parametrize("stat", STATS)
def test_the_map_is_the_definition_in_numpy(case, stat):
    E = handle(case)
    vm = the_map(stat, offset=True)
    m, idx, R = run(E, case, vm)
    E.close()
    ref = xcor.exposed_map_reference(case.pairs_lv, case.ob, case.F, vm)
    assert np.array_equal(np.isnan(m), OUTSIDE) and np.array_equal(np.isnan(ref), OUTSIDE)
    worst, ve = 0.0, np.arange(7)
    for i, j in np.argwhere(~OUTSIDE):
        mom, D = xc.moment_differences(case, case.pairs_lv[idx[i, j], ve])
        assert xcor.cell_value(mom, vm) == ref[i, j]
        rows, small = xc.row_bounds(mom, D, vm)
        print("%s cell (%d, %d): largest relative change %.3e" % (stat, i, j, small))
        assert small < 1e-3, (stat, i, j, small)
        tol = 2.0 * float(np.sum(rows)) + xcor.cell_bound(mom, vm)
        assert tol > 0 and abs(m[i, j] - ref[i, j]) <= tol, (stat, i, j, m[i, j], ref[i, j], tol)
        worst = max(worst, abs(m[i, j] - ref[i, j]) / tol)
    print("%s: worst |map - exposed_map_reference| / tolerance %.3e over the %d inside cells" % (stat, worst, np.count_nonzero(~OUTSIDE)))


def test_cells_do_not_depend_on_the_rest_of_the_call_or_on_the_handles_history(case):
    P = case.P
    E = handle(case)
    plain = Engine(P.static)
    spec_ref = plain.run(P.atm, P.opts)["spectrum"]
    plain.close()
    deep, keep = pc.thinner(P, 1e-3)
    for stat in STATS:
        vm = the_map(stat, offset=True)
        m, idx, R = run(E, case, vm)
        # one cell alone: spans of one lag, R = 7, its rows numbered 0 .. 6
        for i, j in ((2, 3), (5, 2), (0, 0)):
            one, _, r1 = run(E, case, the_map(stat, offset=True, kp=xc.KP[i:i + 1], vsys=xc.VSYS[j:j + 1]))
            assert r1 == 7 and one.shape == (1, 1) and same_bits(one[0, 0], m[i, j]), (stat, i, j)
        # a sub-map: other spans, other bases
        sub, _, rs = run(E, case, the_map(stat, offset=True, kp=xc.KP[1:4], vsys=xc.VSYS[2:]))
        assert 7 < rs < R and same_bits(sub, m[1:4, 2:]), stat
        # the axes reversed: the same spans, every cell at another place of its chunk -- and, in the 143-cell map, in another chunk
        rev, _, rr = run(E, case, the_map(stat, offset=True, kp=xc.KP[::-1], vsys=xc.VSYS[::-1]))
        assert rr == R and same_bits(rev[::-1, ::-1], m), stat
        vm2 = the_map(stat, second=True)
        m2, _, R2 = run(E, case, vm2)
        rev2, _, _ = run(E, case, the_map(stat, second=True, kp=KP2[::-1], vsys=VSYS2[::-1]))
        assert same_bits(rev2[::-1, ::-1], m2), stat
        # a cell of the large map alone, and one shared by the two maps' grids had there been one: the large map's first cell
        one, _, _ = run(E, case, the_map(stat, second=True, kp=KP2[:1], vsys=VSYS2[:1]))
        assert same_bits(one[0, 0], m2[0, 0]), stat
        # after other runs on the handle -- another product, another atmosphere and back --, with and without the extras
        E.run_trail(P.atm, P.opts, LAGS)
        E.run_filtered_moments(deep, P.opts, LAGS[idx[0, 0]])
        E.run_exposed_map(deep, P.opts, vm2)
        a = E.run_exposed_map(P.atm, P.opts, vm)
        b, spec = E.run_exposed_map(P.atm, P.opts, vm, spectrum=True)
        c, idx2, r2, spec2 = E.run_exposed_map(P.atm, P.opts, vm, lag_index=True, nrows=True, spectrum=True)
        for x in (a, b, c):
            assert same_bits(x, m), stat
        assert np.array_equal(idx, idx2) and r2 == R and np.array_equal(spec, spec_ref) and np.array_equal(spec2, spec_ref)
    E.close()


def test_with_a_weighted_filter_a_highpass_and_a_broadening_installed(case):
    P = case.P
    vm, vm2 = the_map("ccf", offset=True), the_map("chi2", second=True)
    E = handle(case)
    plain = run(E, case, vm)[0]
    # the weighted filter in the slot, 3 and 5 components (paddings 4 and 8), over weights with masked entries
    for ncomp in (3, 5):
        ob = xcor.Observed(case.ob.seg_first, case.ob.data, wc.edge_weights(7, len(case.px), ncomp, 200, 210, 220, seed=0), case.ob.gain)
        wf = xcor.WeightedFilter(wc.random_basis(ob.nseg, 7, ncomp, seed=50))
        live = wc.decisive(ob, wf)
        W = Engine(P.static)
        W.set_pixels(case.px)
        W.set_observed(ob)
        assert W.set_weighted_filter(wf) == np.count_nonzero(~live)
        W.set_exposures(table())
        for v in (vm, vm2):
            m, idx, R = run(W, case, v)
            xc.check_contract(case, W, v, m, idx, key="weighted %d" % ncomp, what="weighted filter, %d components" % ncomp)
        W.close()
    E.set_highpass(xcor.gaussian_highpass(6.0))
    for v in (vm, vm2):
        m, idx, R = run(E, case, v)
        xc.check_contract(case, E, v, m, idx, key="highpass", what="high-pass")
    assert np.all(run(E, case, vm)[0][~OUTSIDE] != plain[~OUTSIDE])
    E.set_highpass(None)
    E.set_broadening(broaden.Rotation(4.0, 0.4))
    for v in (vm, vm2):
        m, idx, R = run(E, case, v)
        xc.check_contract(case, E, v, m, idx, key="broadening", what="broadening")
    assert np.all(run(E, case, vm)[0][~OUTSIDE] != plain[~OUTSIDE])
    E.set_highpass(xcor.gaussian_highpass(6.0))
    m, idx, R = run(E, case, vm)
    xc.check_contract(case, E, vm, m, idx, key="highpass and broadening", what="high-pass and broadening")
    E.set_highpass(None)
    E.set_broadening(None)
    assert same_bits(run(E, case, vm)[0], plain)
    E.close()


def test_nothing_else_moves(case):
    P = case.P
    vm = the_map("ccf", offset=True)
    cell = xcor.nearest_lags(vm)[2, 3]

    def neighbours(E, table_runs):
        out = [E.run_filtered_map(P.atm, P.opts, vm), E.run_trail(P.atm, P.opts, LAGS)] + list(E.run_velocity_map(P.atm, P.opts, vm, per=True))
        if table_runs:
            out += list(E.run_filtered_moments(P.atm, P.opts, LAGS[cell], values=True)) + [E.run_exposed(P.atm, P.opts, pc.SHIFTS), E.run_moments(P.atm, P.opts, pc.SHIFTS)]
        return out

    def same(a, b):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))

    bare = handle(case, ex=None)
    without = neighbours(bare, False)
    bare.close()
    E = handle(case)
    before = neighbours(E, True)
    assert same(before[:4], without)                                  # the filtered map, the trail and the velocity map ignore the table
    m = E.run_exposed_map(P.atm, P.opts, vm)
    assert same(neighbours(E, True), before)
    E.run_exposed_map(P.atm, P.opts, the_map("chi2", second=True))
    assert same(neighbours(E, True), before)
    assert same_bits(E.run_exposed_map(P.atm, P.opts, vm), m)
    # the handle's table is the one installed, not the rows' of the last map: another table, another map; the first back, the first map
    E.set_exposures(Exposures(scale=SCALE[::-1].copy()))
    other = E.run_exposed_map(P.atm, P.opts, vm)
    assert np.all(other[~OUTSIDE] != m[~OUTSIDE])
    E.set_exposures(table())
    assert same_bits(E.run_exposed_map(P.atm, P.opts, vm), m) and same(neighbours(E, True), before)
    E.close()


def test_a_map_with_every_cell_outside(case):
    P = case.P
    E = handle(case)
    plain = Engine(P.static)
    spec_ref = plain.run(P.atm, P.opts)["spectrum"]
    plain.close()
    vm = the_map("ccf", offset=True)
    before = E.run_exposed_map(P.atm, P.opts, vm)
    far = the_map("ccf", offset=True, vsys=xc.VSYS + 200.0)
    m, idx, R, spec = E.run_exposed_map(P.atm, P.opts, far, lag_index=True, nrows=True, spectrum=True)
    assert R == 0 == xcor.exposed_map_rows(far)[3] and np.all(np.isnan(m)) and np.array_equal(spec, spec_ref)
    assert np.array_equal(idx, xcor.nearest_lags(far)) and np.all(np.any(idx < 0, axis=-1))
    assert np.all(np.isnan(E.run_exposed_map(P.atm, P.opts, far)))
    assert same_bits(E.run_exposed_map(P.atm, P.opts, vm), before)
    E.close()


def test_refusals(case):
    P, px, ob = case.P, case.px, case.ob
    dp = _abi.c_double_p
    vm = the_map("chi2", offset=True)

    def refusal(E, code=-1):
        with pytest.raises(EngineError) as ei:
            E.run_exposed_map(P.atm, P.opts, vm)
        assert ei.value.code == code
        return str(ei.value)

    E = Engine(P.static)
    assert "trx_run_exposed_map: no observed set installed (trx_set_observed)" in refusal(E)      # no pixel set, no observed set
    E.set_pixels(px)
    assert "trx_run_exposed_map: no observed set installed (trx_set_observed)" in refusal(E)
    assert E.run(P.atm, P.opts)["spectrum"].shape == (P.nwn,)
    E.set_observed(ob)
    assert "trx_run_exposed_map: no filter installed (trx_set_filter)" in refusal(E)
    E.set_exposures(table())
    assert "trx_run_exposed_map: no filter installed (trx_set_filter)" in refusal(E)              # no filter, a table
    assert E.run_exposed(P.atm, P.opts, pc.SHIFTS).shape == (7, 800, 2)
    E.set_exposures(None)
    E.set_filter(case.F)
    assert "trx_run_exposed_map: no exposure table installed (trx_set_exposures)" in refusal(E)   # a filter, no table
    plain = E.run_filtered_map(P.atm, P.opts, vm)
    assert np.array_equal(np.isnan(plain), OUTSIDE)
    E.set_exposures(table())
    before = run(E, case, vm)
    m, idx, nr = np.full((7, 5), -7.0), np.full((7, 5, 7), -7, dtype=np.int32), C.c_int64(-7)
    lib = E._lib

    def raw(c, to_map=m):
        rc = lib.trx_run_exposed_map(E._h, C.byref(P.atm), C.byref(P.opts), None, C.byref(c) if c is not None else None,
                                     to_map.ctypes.data_as(dp) if to_map is not None else None, idx.ctypes.data_as(_abi.c_int32_p), C.byref(nr), None)
        assert np.all(m == -7.0) and np.all(idx == -7) and nr.value == -7      # a refusal touches no output
        return rc, (lib.trx_last_error(E._h) or b"").decode()

    def changed(**fields):
        c = vm.to_c()
        for k, v in fields.items():
            setattr(c, k, v)
        return c

    # a filtered map's refusals, under this call's name
    assert raw(None) == (-1, "trx_run_exposed_map: vm is NULL")
    assert raw(vm.to_c(), to_map=None) == (-1, "trx_run_exposed_map: map is NULL")
    assert raw(changed(nlag=0)) == (-1, "trx_run_exposed_map: nlag < 1")
    assert raw(changed(nlag=2 ** 30)) == (-1, "trx_run_exposed_map: nlag * npix above what one pixel launch takes")
    assert raw(changed(stat=4)) == (-1, "trx_run_exposed_map: unknown stat 4")
    assert raw(changed(kp=None)) == (-1, "trx_run_exposed_map: kp is NULL")
    long_kp, long_vsys = np.full(2 ** 15, 100.0), np.zeros(2 ** 14)
    assert raw(changed(nkp=2 ** 15, nvsys=2 ** 14, kp=long_kp.ctypes.data_as(dp), vsys=long_vsys.ctypes.data_as(dp))) == \
        (-1, "trx_run_exposed_map: nkp * nvsys * nexp above 2^31 - 1")
    # its own: the pairs' bytes.  Two cells at rest at the two ends of a grid of 100 000 lags: every exposure's span is the
    # whole grid, R = 700 000 rows of 800 pixels -- refused behind the tracks, ahead of the pixel pass
    kms = np.linspace(-50.0, 50.0, 100_000)
    wide = xcor.VelocityMap(kms, [0.0], [kms[0], kms[-1]], xc.ORBIT, stat="chi2")
    assert xcor.exposed_map_rows(wide)[3] == 700_000 and 700_000 * 800 * 16 > _abi.EXPOSED_MAP_PAIR_BYTES
    two = np.full((1, 2), -7.0)
    rc = lib.trx_run_exposed_map(E._h, C.byref(P.atm), C.byref(P.opts), None, C.byref(wide.to_c()), two.ctypes.data_as(dp), None, C.byref(nr), None)
    assert rc == -1 and np.all(two == -7.0) and nr.value == -7
    assert (lib.trx_last_error(E._h) or b"").decode() == \
        "trx_run_exposed_map: R = 700000 rows of 800 pixels are 8960000000 bytes of pairs, above kExposedMapPairBytes (8589934592)"
    # the handle is usable and the next run's bits are unchanged; lag_index and nrows may be NULL
    alone = np.zeros((7, 5))
    assert lib.trx_run_exposed_map(E._h, C.byref(P.atm), C.byref(P.opts), None, C.byref(vm.to_c()), alone.ctypes.data_as(dp), None, None, None) == 0
    assert same_bits(alone, before[0])
    assert same_bits(E.run_filtered_map(P.atm, P.opts, vm), plain)
    E.close()
    # a shard's partial pairs say nothing about the live columns or the moments
    n = P.nwn
    try:
        P.set_shard(1000, 3000)
        S = Engine(P.static)
        S.set_pixels(pixels.Pixels([2510.0, 2520.0, 2530.0, 2540.0], [0.2, 0.3, 1.5, 0.4], 4.0))
        S.set_observed(xcor.Observed([0, 1, 4], np.ones((7, 4))))
        S.set_exposures(table())
        assert "trx_run_exposed_map: this handle's shard is not the whole grid" in refusal(S, code=-6)
        assert S.run_exposed(P.atm, P.opts, pc.SHIFTS).shape == (7, 4, 2)
        S.close()
    finally:
        P.set_shard(0, n)


def test_the_batch_form(case):
    P, px, ob = case.P, case.px, case.ob
    dp = _abi.c_double_p
    K = 3
    atms, keep = pc.atmospheres(P, K)
    rot = [broaden.Rotation(4.0, 0.4), broaden.Rotation(2.5, 0.1), broaden.Rotation(6.0, 0.8)]
    tables = [table(), Exposures(scale=SCALE[::-1].copy()), Exposures(smear=np.roll(SMEAR, 2))]
    vm2 = the_map("loglike_bl19", second=True, offset=True)
    E = handle(case)
    one, each = [], []
    for j in range(K):
        E.set_broadening(rot[j])
        E.set_exposures(tables[0])
        one.append(E.run_exposed_map(atms[j], P.opts, vm2))
        E.set_exposures(tables[j])
        each.append(E.run_exposed_map(atms[j], P.opts, vm2))
    E.close()
    assert len({r.tobytes() for r in one}) == K and len({r.tobytes() for r in each}) == K and not same_bits(one[1], each[1])
    B = Batch(P.static, ways=2)
    B.set_pixels(px)

    def refusal():
        with pytest.raises(EngineError) as ei:
            B.run_exposed_map(atms, P.opts, vm2)
        assert ei.value.code == -1
        return str(ei.value)

    assert "trx_run_batch_exposed_map: no observed set installed (trx_batch_set_observed)" in refusal()
    B.set_observed(ob)
    assert "trx_run_batch_exposed_map: no filter installed (trx_batch_set_filter)" in refusal()
    B.set_filter(case.F)
    assert "trx_run_batch_exposed_map: no exposure table installed (trx_batch_set_exposures)" in refusal()       # n = 0
    B.set_broadening(rot)
    B.set_exposures(tables[0])
    for rep in range(2):
        maps = B.run_exposed_map(atms, P.opts, vm2)
        assert maps.shape == (K, vm2.nkp, vm2.nvsys)
        for j in range(K):
            assert same_bits(maps[j], one[j]), (rep, j)
    B.set_exposures(tables)
    for rep in range(2):
        maps = B.run_exposed_map(atms, P.opts, vm2)
        for j in range(K):
            assert same_bits(maps[j], each[j]), (rep, j)
    B.set_exposures(tables[:2])
    assert "trx_run_batch_exposed_map: 2 exposure tables installed (trx_batch_set_exposures) for 3 atmospheres" in refusal()
    B.set_exposures(tables)
    out = np.full((K, vm2.nkp, vm2.nvsys), -7.0)
    arr = (_abi.TrxAtm * K)(*atms)
    lib = B._lib

    def batch(c, ptrs):
        rc = lib.trx_run_batch_exposed_map(B._b, K, arr, C.byref(P.opts), C.byref(c) if c is not None else None, (dp * K)(*ptrs))
        assert np.all(out == -7.0)
        return rc, (lib.trx_last_error(None) or b"").decode()

    ptrs = [out[j].ctypes.data_as(dp) for j in range(K)]
    assert batch(vm2.to_c(), [ptrs[0], None, ptrs[2]]) == (-1, "trx_run_batch_exposed_map: map[1] is NULL")
    assert batch(None, ptrs) == (-1, "trx_run_batch_exposed_map: vm is NULL")
    c = vm2.to_c()
    c.stat = 9
    assert batch(c, ptrs) == (-1, "trx_run_batch_exposed_map: unknown stat 9")
    assert same_bits(B.run_exposed_map(atms, P.opts, vm2), maps)
    # the filtered map of the batch keeps ignoring the tables
    E = handle(case, ex=None)
    E.set_broadening(rot[1])
    assert same_bits(B.run_filtered_map(atms, P.opts, vm2)[1], E.run_filtered_map(atms[1], P.opts, vm2))
    E.close()
    B.close()
