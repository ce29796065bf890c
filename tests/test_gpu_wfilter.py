"""The weighted detrending filter on the device (trx_set_weighted_filter / trx_batch_set_weighted_filter and the filtered
runs behind it, include/transit_hip.h) against transit_amd.xcor's mirror of the same definition, BIT FOR BIT.

The case is xcor_checks': pixel_cases.make("eclipse", 20 000 lines, 6001 bins), the 800 pixels with their two off-grid
ones (b = 0 at every exposure), 7 exposures, the segments [1, 63, 64, 65, 200, 0, 7, 400] -- a tile of one lane, 64 + 1, an
empty segment, ordinary ones -- and ncomp 1, 3, 5 and 9: the kernels' paddings 4, 8 and 16.  The weights are
wfilter_cases.edge_weights: a column masked at every exposure (MASKED), one with exactly ncomp - 1 positive weights (SHORT,
singular), one with exactly ncomp (EXACT, live), and single masked entries in a tenth of the other columns.  With 9
components and 7 exposures every column is singular: the <16> kernels are held on live columns by a further case of 12
exposures.  Before any device call every test asserts wfilter_cases.decisive on the host: no pivot of the case lies between
2^-40 and 2^-12 of its diagonal entry, so that no live/dead decision hinges on a pivot's last bits.

Values and flags are compared in bits.  The moments follow xcor_checks.check_filtered_moments' rule over the values the device returned;
the map follows xcor_checks.check_contract, xcor.cell_value of the moments within xcor.cell_bound."""
import ctypes as C

import numpy as np
import pytest

import pixel_cases as pc
import wfilter_cases as wc
import xcor_checks as xc
from bits import same_bits
from transit_amd import exposures, xcor
from transit_amd.engine import Batch, Engine, EngineError

pytestmark = pytest.mark.gpu

SHIFTS = pc.SHIFTS
LAGS = xc.LAGS
MASKED, SHORT, EXACT = 200, 210, 220             # edge columns, in the segment of 200 pixels
NCOMPS = (1, 3, 5, 9)
EPS = 2.0 ** -52


class Case:
    def __init__(self, P, px, scale, pairs):
        self.P, self.px, self.scale, self.pairs = P, px, scale, pairs
        self.sets = {}

    def the_set(self, ncomp, nexp=7):
        """(observed set, weighted filter, the mirror's live flags) for ncomp components, made once; the precondition
        is asserted here, on the host, before anything of it reaches the device"""
        if (ncomp, nexp) not in self.sets:
            base = xc.observed(len(self.px), self.scale, nexp=nexp)
            ob = xcor.Observed(base.seg_first, base.data, wc.edge_weights(nexp, len(self.px), ncomp, MASKED, SHORT, EXACT, seed=0), base.gain)
            wf = xcor.WeightedFilter(wc.random_basis(ob.nseg, nexp, ncomp, seed=50))
            self.sets[(ncomp, nexp)] = (ob, wf, wc.decisive(ob, wf))
        return self.sets[(ncomp, nexp)]

    def handle(self, ncomp=None):
        E = Engine(self.P.static)
        E.set_pixels(self.px)
        if ncomp is not None:
            ob, wf, live = self.the_set(ncomp)
            E.set_observed(ob)
            assert E.set_weighted_filter(wf) == np.count_nonzero(~live)
        return E


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    P = pc.make(tmp_path_factory.mktemp("wfilter"), "eclipse", nlines=20_000)
    px = xc.pixel_set(P)
    E = Engine(P.static)
    scale = float(np.mean(E.run(P.atm, P.opts)["spectrum"]))
    E.set_pixels(px)
    pairs = E.run_pixels(P.atm, P.opts, SHIFTS)
    E.close()
    assert pairs.shape == (7, 800, 2)
    for p in xc.OFF_GRID:
        assert np.all(pairs[:, p, 1] == 0)
    return Case(P, px, scale, pairs)


def check_edges(val, ob, live, ncomp):
    """the NaN pattern: the pivot rule's dead columns and the off-grid pixels, nothing else"""
    dead = ~live
    dead[list(xc.OFF_GRID)] = True
    assert np.array_equal(np.isnan(val).any(axis=0), dead) and np.isnan(val[:, dead]).all()
    assert not live[MASKED] and not live[SHORT] and bool(live[EXACT]) == (ncomp <= ob.nexp)
    assert np.count_nonzero(ob.weight[:, SHORT] > 0) == (ncomp - 1 if ncomp - 1 <= ob.nexp else 0)
    assert np.count_nonzero(ob.weight[:, EXACT] > 0) == min(ncomp, ob.nexp)
    if ncomp <= ob.nexp:
        one = (np.count_nonzero(ob.weight == 0, axis=0) == 1) & live
        assert np.count_nonzero(live) == ob.npix - 2 and np.count_nonzero(one) > 40 and live[0] and live[192]
    else:
        assert not live.any()


@pytest.mark.parametrize("ncomp", NCOMPS)
def test_values_flags_and_moments_are_the_mirrors(case, ncomp):
    P = case.P
    ob, wf, live = case.the_set(ncomp)
    E = case.handle(ncomp)
    assert np.array_equal(E.run_pixels(P.atm, P.opts, SHIFTS), case.pairs)
    mom, val = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    ref = xcor.weighted_filter_reference(case.pairs, ob, wf)
    assert same_bits(val, ref), "ncomp %d" % ncomp
    check_edges(val, ob, live, ncomp)
    xc.check_weighted_moments(mom, val, ob, "weighted, ncomp %d" % ncomp)
    assert np.array_equal(E.run_filtered_moments(P.atm, P.opts, SHIFTS), mom)
    # behind an exposure table and a high-pass: the mirror over their pairs
    ex = exposures.Exposures(np.array([1.0, 0.5, 2.0, -0.25, 1.0, 3.0, 1e-3]), np.array([0.0, 2e-9, 1e-6, 3e-6, 1.3e-5, 0.0, 1e-5]))
    hp = xcor.gaussian_highpass(6.0)
    E.set_exposures(ex)
    E.set_highpass(hp)
    exposed = E.run_exposed(P.atm, P.opts, SHIFTS)
    assert not np.array_equal(exposed, case.pairs)
    hval = xcor.highpass_reference(exposed, ob, hp)
    gain_free = xcor.Observed(ob.seg_first, ob.data, ob.weight, None)
    mom2, val2 = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    assert same_bits(val2, xcor.weighted_filter_reference(xcor.highpass_pairs(hval), gain_free, wf)), "ncomp %d, exposed and high-passed" % ncomp
    xc.check_weighted_moments(mom2, val2, ob, "weighted behind the exposure table and the high-pass, ncomp %d" % ncomp)
    if ncomp <= 7:
        assert not np.array_equal(mom2, mom)
    E.set_exposures(None)
    E.set_highpass(None)
    assert np.array_equal(E.run_filtered_moments(P.atm, P.opts, SHIFTS), mom)
    E.close()


def test_nine_components_of_twelve_exposures_are_live(case):
    """the <16> instantiations on live columns: 9 components, 12 exposures"""
    P = case.P
    shifts = np.concatenate([SHIFTS, SHIFTS[:5] * (1.0 + 2e-5)])
    ob, wf, live = case.the_set(9, nexp=12)
    assert np.count_nonzero(live) == 798 and live[EXACT]
    E = Engine(P.static)
    E.set_pixels(case.px)
    E.set_observed(ob)
    assert E.set_weighted_filter(wf) == 2
    pairs = E.run_pixels(P.atm, P.opts, shifts)
    mom, val = E.run_filtered_moments(P.atm, P.opts, shifts, values=True)
    assert same_bits(val, xcor.weighted_filter_reference(pairs, ob, wf))
    check_edges(val, ob, live, 9)
    xc.check_weighted_moments(mom, val, ob, "weighted, 9 components of 12 exposures")
    E.close()


def test_a_masked_entry_matters_and_equal_weights_are_the_plain_filter(case):
    P = case.P
    base = xc.observed(len(case.px), case.scale)
    seg = base.seg_first
    w = np.ones_like(base.data)
    w[:, seg[4]:seg[5]] = 0.75                           # a segment whose weights are all equal, and not 1
    col = int(seg[7]) + 100
    w[3, col] = 0.0                                      # one masked exposure in an otherwise ordinary column
    ob = xcor.Observed(seg, base.data, w, base.gain)
    F = xcor.svd_filter(ob.data, seg, 3)
    wf = xcor.WeightedFilter(xcor.svd_basis(ob.data, seg, 3))
    live = wc.decisive(ob, wf)
    assert not live[0] and live[1:].all()                # (the segment of one pixel has one singular vector, not three)
    E = Engine(P.static)
    E.set_pixels(case.px)
    E.set_observed(ob)
    E.set_filter(F)
    plain = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)[1]
    assert E.set_weighted_filter(wf) == 1
    weighted = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)[1]
    E.close()
    assert same_bits(weighted, xcor.weighted_filter_reference(case.pairs, ob, wf))
    tol = xcor.weighted_filter_bound(case.pairs, ob, wf) + (ob.nexp + F.ncomp + 8) * EPS * xcor.filter_abs_reference(case.pairs, ob, F)
    same = np.ones(ob.npix, dtype=bool)
    same[[0, col] + list(xc.OFF_GRID)] = False
    diff = np.abs(weighted - plain)
    assert np.all(diff[:, same] <= tol[:, same])
    print("equal weights: worst |weighted - plain| / (sum of the two bounds) %.4f" % float(np.max(diff[:, same] / tol[:, same])))
    assert np.all(diff[:, col] > 1e3 * tol[:, col])
    print("one masked entry: |weighted - plain| is at least %.3g times the bounds' sum in that column" % float(np.min(diff[:, col] / tol[:, col])))


@pytest.mark.parametrize("ncomp", [3, 9])
def test_filtered_map_cells_are_the_filtered_moments(case, ncomp):
    P = case.P
    ob, wf, live = case.the_set(ncomp)
    E = case.handle(ncomp)
    moms = {}

    def moments(idx):
        key = np.asarray(idx, dtype=np.int64).tobytes()
        if key not in moms:
            moms[key] = E.run_filtered_moments(P.atm, P.opts, LAGS[idx])
        return moms[key]

    for stat in xc.STATS:
        vm = xc.the_filtered_map(stat, offset=True)
        m, idx = E.run_filtered_map(P.atm, P.opts, vm, lag_index=True)
        assert np.array_equal(idx, xcor.nearest_lags(vm)) and np.array_equal(np.isnan(m), xc.OUTSIDE)
        differ = 0
        for i, j in np.argwhere(~xc.OUTSIDE):
            mom = moments(idx[i, j])
            want, bound = xcor.cell_value(mom, vm), xcor.cell_bound(mom, vm)
            if ncomp <= 7:
                assert np.isfinite(m[i, j]) and bound > 0 and abs(m[i, j] - want) <= bound, (stat, i, j, m[i, j], want, bound)
            else:                                            # every column dead: no pixel in any row
                assert np.all(mom == 0) and m[i, j] == want, (stat, i, j, m[i, j], want)
            differ += not same_bits(m[i, j], want)
        print("ncomp %d, %s: %d of 28 cells differ in bits from cell_value(run_filtered_moments)" % (ncomp, stat, differ))
        # a cell's bits do not depend on its chunk or its place there: one cell alone, and the axes reversed
        for i, j in ((2, 3), (0, 0)):
            one = E.run_filtered_map(P.atm, P.opts, xc.the_filtered_map(stat, offset=True, kp=xc.KP[i:i + 1], vsys=xc.VSYS[j:j + 1]))
            assert one.shape == (1, 1) and same_bits(one[0, 0], m[i, j]), (stat, i, j)
    if ncomp == 3:
        # the definition in numpy, moments by fsum: on the pairs of the lags, to the cell bound and the moments' rule
        vm = xc.the_filtered_map("chi2", offset=True)
        lag_pairs = E.run_pixels(P.atm, P.opts, LAGS)
        m, idx = E.run_filtered_map(P.atm, P.opts, vm, lag_index=True)
        i, j = 2, 3
        val = xcor.weighted_filter_reference(lag_pairs[idx[i, j]], ob, wf)
        xc.check_weighted_moments(moments(idx[i, j]), val, ob, "the cell (2, 3): moments of the mirror's values")
        # 143 cells: three chunks with a ragged last one; reversed, every cell sits in another chunk
        vm2 = xc.the_filtered_map("ccf", second=True)
        m2 = E.run_filtered_map(P.atm, P.opts, vm2)
        rev2 = E.run_filtered_map(P.atm, P.opts, xc.the_filtered_map("ccf", second=True, kp=xc.FMAP_KP2[::-1], vsys=xc.FMAP_VSYS2[::-1]))
        assert m2.size > 2 * xc.CHUNK and m2.size % xc.CHUNK != 0
        assert same_bits(rev2[::-1, ::-1], m2) and np.count_nonzero(np.isfinite(m2)) > xc.CHUNK
    E.close()


def test_batch_moments_and_maps_are_the_single_handles(case):
    P = case.P
    ob, wf, live = case.the_set(5)
    K = 3
    atms, keep = pc.atmospheres(P, K)
    shifts = np.stack([np.roll(SHIFTS, j) * (1.0 + 1e-6 * j) for j in range(K)])
    vm = xc.the_filtered_map("loglike_bl19", offset=True)
    E = case.handle(5)
    ref = np.stack([E.run_filtered_moments(atms[j], P.opts, shifts[j]) for j in range(K)])
    maps = np.stack([E.run_filtered_map(atms[j], P.opts, vm) for j in range(K)])
    E.close()
    assert len({ref[j].tobytes() for j in range(K)}) == K and len({maps[j].tobytes() for j in range(K)}) == K
    B = Batch(P.static, ways=2)
    B.set_pixels(case.px)
    with pytest.raises(EngineError) as ei:                 # nothing to install it over: on no handle
        B.set_weighted_filter(wf)
    assert ei.value.code == -1 and "weighted filter: no observed set installed" in str(ei.value)
    B.set_observed(ob)
    with pytest.raises(EngineError) as ei:
        B.run_filtered_moments(atms, P.opts, shifts)
    assert "no filter installed" in str(ei.value)
    B.set_weighted_filter(wf)
    for rep in range(2):
        assert np.array_equal(B.run_filtered_moments(atms, P.opts, shifts), ref), rep
        assert same_bits(B.run_filtered_map(atms, P.opts, vm), maps), rep
    bad = wf.basis.copy()
    bad[4, 2, 1] = np.inf
    with pytest.raises(EngineError) as ei:                 # refused on every handle: the one installed stays
        B.set_weighted_filter(xcor.WeightedFilter(bad))
    assert ei.value.code == -1 and "segment 4" in str(ei.value)
    assert np.array_equal(B.run_filtered_moments(atms, P.opts, shifts), ref)
    B.set_weighted_filter(None)
    with pytest.raises(EngineError) as ei:
        B.run_filtered_map(atms, P.opts, vm)
    assert "no filter installed" in str(ei.value)
    B.close()


def test_lifetimes_and_refusals(case):
    P = case.P
    ob, wf, live = case.the_set(3)
    F = xc.random_filter(ob.nseg, 3, ob.nexp, seed=1)
    E = Engine(P.static)
    lib = E._lib

    def refusal(w):
        with pytest.raises(EngineError) as ei:
            E.set_weighted_filter(w)
        assert ei.value.code == -1
        return str(ei.value)

    assert "weighted filter: no observed set installed (trx_set_observed)" in refusal(wf)      # no pixel set, no observed set
    E.set_pixels(case.px)
    assert "no observed set installed" in refusal(wf)
    E.set_observed(ob)
    with pytest.raises(EngineError) as ei:
        E.run_filtered_moments(P.atm, P.opts, SHIFTS)
    assert ei.value.code == -1 and "no filter installed" in str(ei.value)
    nsing = E.set_weighted_filter(wf)
    assert nsing == np.count_nonzero(~live) == 2
    weighted = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    # the slot is one: the plain filter replaces the weighted one, and the reverse, each with exactly its own bits
    E.set_filter(F)
    plain = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    bare = Engine(P.static)
    bare.set_pixels(case.px)
    bare.set_observed(ob)
    bare.set_filter(F)
    want = bare.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    bare.close()
    assert np.array_equal(plain[0], want[0]) and same_bits(plain[1], want[1]) and not same_bits(plain[1], weighted[1])
    assert E.set_weighted_filter(wf) == nsing

    def unchanged(what):
        got = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
        assert np.array_equal(got[0], weighted[0]) and same_bits(got[1], weighted[1]), what

    unchanged("installed again")
    # every refusal names its reason and leaves the filter in force

    def changed(idx, x):
        b = wf.basis.copy()
        b[idx] = x
        return xcor.WeightedFilter(b)

    for what, w, name in (("nan", changed((1, 0, 2), np.nan), "segment 1: basis entry must be finite"),
                          ("inf", changed((0, 6, 0), np.inf), "segment 0: basis entry must be finite"),
                          ("-inf", changed((7, 3, 1), -np.inf), "segment 7: basis entry must be finite"),
                          ("17 components", xcor.WeightedFilter(np.ones((8, 7, 17))), "ncomp above TRX_FILTER_MAX (16)")):
        assert name in refusal(w), what
        unchanged(what)

    def raw(**kw):
        c = wf.to_c()
        for k, v in kw.items():
            setattr(c, k, v)
        n = C.c_int64(-7)
        return lib.trx_set_weighted_filter(E._h, C.byref(c), C.byref(n)), lib.trx_last_error(E._h)

    assert raw(ncomp=-1) == (-1, b"weighted filter: ncomp < 0")
    assert raw(ncomp=17)[0] == -1 and b"TRX_FILTER_MAX" in raw(ncomp=17)[1]
    assert raw(basis=None) == (-1, b"weighted filter: NULL basis array")
    unchanged("raw refusals")
    assert lib.trx_set_weighted_filter(E._h, C.byref(wf.to_c()), None) == 0        # nsingular may be NULL
    unchanged("without nsingular")
    # a refused plain filter leaves the weighted one in force too
    with pytest.raises(EngineError):
        E.set_filter(xc.random_filter(ob.nseg, 17, ob.nexp, seed=2))
    unchanged("a refused plain filter")
    # and a refused weighted filter leaves a plain one in force
    E.set_filter(F)
    assert "segment 1" in refusal(changed((1, 0, 2), np.nan))
    assert np.array_equal(E.run_filtered_moments(P.atm, P.opts, SHIFTS), plain[0])
    # cleared, by None and by ncomp = 0; dropped by set_observed and by set_pixels
    vm = xc.the_filtered_map("ccf", offset=True)
    for clear in ("none", "ncomp 0", "set_observed", "set_pixels"):
        assert E.set_weighted_filter(wf) == nsing
        if clear == "none":
            assert E.set_weighted_filter(None) == 0
        elif clear == "ncomp 0":
            assert raw(ncomp=0)[0] == 0
        elif clear == "set_observed":
            E.set_observed(ob)
        else:
            E.set_pixels(case.px)
            E.set_observed(ob)
        with pytest.raises(EngineError) as ei:
            E.run_filtered_moments(P.atm, P.opts, SHIFTS)
        assert ei.value.code == -1 and "no filter installed" in str(ei.value), clear
        with pytest.raises(EngineError) as ei:
            E.run_filtered_map(P.atm, P.opts, vm)
        assert ei.value.code == -1 and "no filter installed" in str(ei.value), clear
    assert E.set_weighted_filter(wf) == nsing
    unchanged("after the clearings")
    # weights NULL: all 1
    E.set_observed(xcor.Observed(ob.seg_first, ob.data, None, ob.gain))
    ones = xcor.Observed(ob.seg_first, ob.data, np.ones_like(ob.data), ob.gain)
    assert wc.decisive(ones, wf).all()
    assert E.set_weighted_filter(wf) == 0
    val = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)[1]
    assert same_bits(val, xcor.weighted_filter_reference(case.pairs, ones, wf))
    E.close()


def test_no_leak_into_other_runs(case):
    """a handle with a plain filter and a handle with none give the bits of handles made the same way that never saw the
    new calls -- with a weighted filter installed, run and cleared on them in between, and one installed elsewhere"""
    P = case.P
    ob, wf, live = case.the_set(5)
    F = xc.random_filter(ob.nseg, 5, ob.nexp, seed=3)
    vm = xc.the_filtered_map("ccf", offset=True)
    elsewhere = case.handle(5)
    elsewhere.run_filtered_moments(P.atm, P.opts, SHIFTS)

    def make(filt):
        E = Engine(P.static)
        E.set_pixels(case.px)
        E.set_observed(ob)
        if filt:
            E.set_filter(F)
        return E

    def runs(E, filt):
        out = [E.run_moments(P.atm, P.opts, SHIFTS), E.run_trail(P.atm, P.opts, LAGS)]
        out += list(E.run_velocity_map(P.atm, P.opts, vm, per=True))
        if filt:
            out += list(E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)) + [E.run_filtered_map(P.atm, P.opts, vm)]
        return out

    for filt in (True, False):
        ref, E = make(filt), make(filt)
        want = runs(ref, filt)
        # the new calls in between: installed, run both ways, and the slot as it was put back
        E.set_weighted_filter(wf)
        E.run_filtered_moments(P.atm, P.opts, SHIFTS)
        with_weighted = [E.run_moments(P.atm, P.opts, SHIFTS), E.run_trail(P.atm, P.opts, LAGS)] + list(E.run_velocity_map(P.atm, P.opts, vm, per=True))
        for a, b in zip(with_weighted, want):
            assert same_bits(a, b), filt                   # (moments, trail and velocity map ignore the slot's content)
        E.run_filtered_map(P.atm, P.opts, vm)
        if filt:
            E.set_filter(F)
        else:
            E.set_weighted_filter(None)
        got = runs(E, filt)
        assert len(got) == len(want) == (7 if filt else 4)
        for a, b in zip(got, want):
            assert same_bits(a, b), filt
        ref.close(); E.close()
    elsewhere.close()
