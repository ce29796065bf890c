"""The observed-set products on the device past 64 exposures and past 64 segments: moments, trail, Kp-Vsys map, plain and
weighted filter, the per-cell maps, SYSREM, PCA, the scatter weights, the data-side high-pass and the normalisation
(include/transit_hip.h) against transit_amd.xcor at the sets of many_cases.py.

The other device tests of this chain run at 4 to 12 exposures and at most 12 segments, on xcor_checks.pixel_set's 800 pixels in
segments of at most 400; orders of a detector's length -- 1024, 1025 and 2049 pixels -- are tests/test_gpu_long_orders.py's,
on many_cases.long_set under the same checkers.  Here the pixel set and the segments stay xcor_checks' and the other two
axes grow:
  - 64, 65 and 130 exposures.  A wave takes the exposures 64 at a time in k_velocity_map and k_cell_stat (the in-order sum
    carried from trip to trip) and in k_sysrem_close's store of the basis; the column kernels take them 4 at a time
    (k_pixel_filter, k_cell_filter, k_pixel_wfilter, k_cell_wfilter, k_wfilter_factor) or 8 at a time (k_sysrem_cols,
    k_sysrem_subtract) with a clamped ragged last trip: 64 is a multiple of both and exactly one wave, 65 = 16 x 4 + 1 =
    8 x 8 + 1 one past all three, 130 two waves and a ragged third; k_trail_moments<2, 4>'s last exposure tile is ragged at
    65 and 130.  ncomp 4, 8 and 16 fill the kernels' register arrays with no zero-padded component, 3, 5 and 6 do not;
  - 64, 65 and 130 segments of 5 exposures: k_trail_stat takes the segments 64 at a time and skips undefined statistics,
    k_cell_stat's per-exposure loop over the segments is long.
What runs on the two axes: moments, trail, velocity map, plain and weighted filter, filtered and exposed map, SYSREM (with
and without injection) and, of the data-side calls, weigh_observed (raw and detrended data, both kinds, clip 3),
highpass_observed (halves 5 and 70) and normalise_observed (MEDIAN_RATIO, and quantile 0.9 + divide + clip 3), all in their
mirrors' bits; pca_observed at 64 and 65 exposures ((5, 8) and (16, 8); 130 is above TRX_PCA_MAX_EXP and refused) and on the
orders sets, where the empty segments on both sides of index 64 and the dead segment give +0 medians, a zero basis without
a sign bit, nwhole 0 and untouched data.

No tolerance here is this file's own.  Every comparison is "the same bits" or one of the derived rules of the tests this
file borrows its checkers from, evaluated at the set's nexp, ncomp and longest segment: xcor_checks.check_moments and
xcor_checks.check_trail ((n_max + 16) * 2^-52 of the absolute sums), xcor_checks.check_per (xcor.per_bound),
xcor_checks.check_values and check_filtered_moments ((nexp + ncomp + 8) * 2^-52 of A), xcor_checks.check_contract
(xcor.cell_bound), the propagation of xcor_checks.row_bounds' docstring for the maps against numpy alone, and
observed_cases.check_sysrem_outputs, observed_cases.check_pca_outputs, observed_cases.check_scatter_outputs, observed_cases.check_normalised
and test_gpu_hpdata's rule (bits).  tests/test_many_cases_host.py holds the preconditions of the sets on the host."""
import numpy as np
import pytest

import hpdata_cases as hc
import many_cases as mc
import normalise_cases as nc
import observed_cases as oc
import pixel_cases as pc
import scatter_cases as cs
import wfilter_cases as wc
import xcor_checks as xc
from bits import same_bits
from transit_amd import xcor
from transit_amd.engine import Batch, Engine, EngineError

pytestmark = pytest.mark.gpu

STATS = xc.STATS
LAGS = mc.LAGS


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    P = pc.make(tmp_path_factory.mktemp("many"), "eclipse", nlines=20_000)
    E = Engine(P.static)
    spec = E.run(P.atm, P.opts)["spectrum"]
    E.close()
    return oc.ManyCase(P, float(np.mean(spec)), spec)


# ---- many exposures ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nexp", mc.NEXPS)
def test_moments_and_trail(case, nexp):
    ms, px, ob = case.exposures(nexp)
    E = case.handle(px, ob)
    oc.check_moments_and_trail(case, E, ms, ob)
    E.close()


@pytest.mark.parametrize("nexp", mc.NEXPS)
def test_velocity_map(case, nexp):
    P = case.P
    ms, px, ob = case.exposures(nexp)
    E = case.handle(px, ob)
    got = oc.check_velocity_map(case, E, ms, E.run_trail(P.atm, P.opts, LAGS))
    if nexp > 64:
        # an exposure below 64 exchanged with one above it, orbit and data together: the same terms in another order, other bits
        a, b = 10, {65: 64, 130: 100}[nexp]
        sw = ms.swapped(a, b)
        perm = np.arange(nexp)
        perm[[a, b]] = perm[[b, a]]
        E.set_observed(sw.observed(case.scale))
        vm = sw.the_map("ccf")
        m, per = E.run_velocity_map(P.atm, P.opts, vm, per=True)
        assert same_bits(per, got["ccf"][1][:, perm])
        assert same_bits(m, xcor.map_from_per(per, vm)) and np.array_equal(np.isnan(m), oc.MANY_OUTSIDE)
        differ = np.count_nonzero(m[~oc.MANY_OUTSIDE] != got["ccf"][0][~oc.MANY_OUTSIDE])
        print("%s: exposures %d and %d exchanged: %d of 11 cells change their bits" % (ms.name, a, b, differ))
        assert differ > 0
    E.close()


@pytest.mark.parametrize("ncomp", [3, 8, 16])
@pytest.mark.parametrize("nexp", mc.NEXPS)
def test_plain_filter(case, nexp, ncomp):
    P = case.P
    ms, px, ob = case.exposures(nexp)
    E = case.handle(px, ob)
    F = xc.random_filter(ob.nseg, ncomp, nexp, seed=ncomp)
    E.set_filter(F)
    what = "%s, plain filter of %d" % (ms.name, ncomp)
    pairs = E.run_pixels(P.atm, P.opts, ms.shifts)
    mom, val = E.run_filtered_moments(P.atm, P.opts, ms.shifts, values=True)
    xc.check_values(val, pairs, ob, F, what)
    assert np.flatnonzero(np.isnan(val).any(axis=0)).tolist() == sorted(ms.off_grid) and np.isnan(val[:, sorted(ms.off_grid)]).all()
    xc.check_filtered_moments(mom, val, ob, what)
    E.close()


@pytest.mark.parametrize("ncomp", [4, 8, 16, 5])
@pytest.mark.parametrize("nexp", [65, 130])
def test_weighted_filter(case, nexp, ncomp):
    P = case.P
    ms, px, ob = case.exposures(nexp)
    E = case.handle(px, ob)
    wf = xcor.WeightedFilter(wc.random_basis(ob.nseg, nexp, ncomp, seed=50 + ncomp))
    live = xcor.weighted_factor(ob, wf)[2]
    assert E.set_weighted_filter(wf) == np.count_nonzero(~live) >= 1
    pairs = E.run_pixels(P.atm, P.opts, ms.shifts)
    mom, val = E.run_filtered_moments(P.atm, P.opts, ms.shifts, values=True)
    assert same_bits(val, xcor.weighted_filter_reference(pairs, ob, wf)), (nexp, ncomp)
    dead = ~live
    dead[list(ms.off_grid)] = True
    assert np.array_equal(np.isnan(val).any(axis=0), dead) and np.isnan(val[:, dead]).all() and dead[ms.masked_col]
    assert np.count_nonzero(dead) < ms.npix // 4
    xc.check_weighted_moments(mom, val, ob, "%s, weighted filter of %d" % (ms.name, ncomp))
    E.close()


@pytest.mark.parametrize("which", ["plain 6", "plain 16", "weighted 8"])
@pytest.mark.parametrize("nexp", mc.NEXPS)
def test_filtered_map(case, nexp, which):
    oc.check_filtered_map(case, *case.exposures(nexp), which)


@pytest.mark.parametrize("which", ["plain 6", "plain 16", "weighted 8"])
@pytest.mark.parametrize("nexp", mc.NEXPS)
def test_exposed_map(case, nexp, which):
    """the table has scale 0 on both sides of exposure 64"""
    P = case.P
    ms, px, ob = case.exposures(nexp)
    E = case.handle(px, ob)
    F = oc.install(E, ob, which)
    E.set_exposures(ms.table())
    C = oc.Cells(P, ob, F, pairs_lv=np.stack([E.run_exposed(P.atm, P.opts, np.full(nexp, s)) for s in LAGS]))
    zero = np.flatnonzero(ms.scale == 0)
    assert np.all(C.pairs_lv[:, zero, :, 0] == 0) and np.all(C.pairs_lv[:, np.flatnonzero(ms.scale != 0)][:, :, 0, 0] != 0)
    for stat in STATS:
        vm = ms.the_map(stat)
        m, idx, R = E.run_exposed_map(P.atm, P.opts, vm, lag_index=True, nrows=True)
        assert R == xcor.exposed_map_rows(vm)[3] and nexp <= R < nexp * LAGS.size
        oc.check_map(E, C, ms, vm, m, idx, "%s, %s, exposed map" % (ms.name, which), key="table")
        if stat == "ccf":
            ref = xcor.exposed_map_reference(C.pairs_lv, ob, F, vm)
            assert np.array_equal(np.isnan(ref), oc.MANY_OUTSIDE) and all(ref[c] == xcor.cell_value(C.reference(idx[c])[0], vm) for c in oc.MANY_INSIDE)
            plain = E.run_filtered_map(P.atm, P.opts, vm)      # the table matters
            assert np.all(plain[~oc.MANY_OUTSIDE] != m[~oc.MANY_OUTSIDE])
    E.close()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ncomp,niter", mc.SYSREM_PAIRS)
@pytest.mark.parametrize("nexp", mc.NEXPS)
def test_sysrem(case, nexp, ncomp, niter, weighted):
    ms, px, full = case.exposures(nexp)
    ob = full if weighted else ms.observed(case.scale, weighted=False)
    E = case.handle(px, ob)
    what = "%s, %d components of %d alternations, %s" % (ms.name, ncomp, niter, "edge weights" if weighted else "no weights")
    D = E.detrend_observed(ncomp, niter)
    mirror = xcor.sysrem_reference(ob.data, ob.weight, ob.seg_first, ncomp, niter)
    oc.check_sysrem_outputs(D, mirror, ob, what)
    assert np.all(D.basis[5] == 0) and np.all(np.any(D.basis[[0, 1, 2, 3, 4, 6, 7], :, 0] != 0, axis=1)), what
    if weighted:
        row = D.basis[ms.masked_seg, ms.masked_exp]
        assert np.all(row == 0) and not np.signbit(row).any(), what
        assert np.array_equal(D.data[ms.masked_exp, ms.segment(ms.masked_seg)], ob.data[ms.masked_exp, ms.segment(ms.masked_seg)]), what
        assert np.all(D.coef[:, ms.masked_col] == 0) and D.nsingular >= 1, what
    print("%s: basis, coef, data and nsingular (%d) are the mirror's" % (what, D.nsingular))
    E.close()


@pytest.mark.parametrize("nexp", mc.NEXPS)
def test_sysrem_with_injection_and_what_it_installs(case, nexp):
    """8 components of 10 alternations with the model injected under the exposure table; the filter the call installs gives
    run_filtered_moments the bits of a fresh handle with the mirror's basis over the mirror's residuals"""
    P = case.P
    ms, px, ob = case.exposures(nexp)
    E = case.handle(px, ob)
    E.set_exposures(ms.table())
    pairs = E.run_exposed(P.atm, P.opts, ms.shifts)
    p0, p1 = 0.05 / case.scale, 0.9
    f0 = xcor.inject_reference(pairs, ob, p0, p1)
    on = pairs[..., 1] > 0
    assert np.count_nonzero(on) == nexp * 798 and np.all(f0[on] != ob.data[on])
    basis, coef, resid = xcor.sysrem_reference(f0, ob.weight, ob.seg_first, 8, 10)
    D = E.detrend_observed(8, 10, inject=(P.atm, P.opts, ms.shifts, p0, p1))
    oc.check_sysrem_outputs(D, (basis, coef, resid), ob, "%s, injected under the table" % ms.name)
    assert np.array_equal(D.spectrum, case.spec)
    got = E.run_filtered_moments(P.atm, P.opts, ms.shifts, values=True)
    E.close()
    F = case.handle(px, xcor.Observed(ob.seg_first, resid, ob.weight, ob.gain))
    assert F.set_weighted_filter(xcor.WeightedFilter(basis)) == D.nsingular
    F.set_exposures(ms.table())
    want = F.run_filtered_moments(P.atm, P.opts, ms.shifts, values=True)
    F.close()
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert np.count_nonzero(np.isfinite(got[1]).all(axis=0)) > 600 and np.isnan(got[1][:, ms.masked_col]).all()


# ---- many exposures: the data-side calls -------------------------------------------------------------------------------
def weigh_raw_and_detrended(E, ob, ncomp, niter, what):
    """weigh_observed on the raw data and on the residuals of detrend_observed(ncomp, niter), both kinds, clip 3: the mirror's
    variance, median, weights, nmasked and nsingular; returns the results of the raw stage"""
    raw = []
    for stage in ("raw", "detrended"):
        D = E.detrend_observed(ncomp, niter) if stage == "detrended" else None
        data = D.data if D else ob.data
        for kind in cs.KINDS:
            mirror = xcor.scatter_reference(data, ob.weight, ob.seg_first, kind, 3.0, 2)
            R = E.weigh_observed(kind, clip=3.0)
            oc.check_scatter_outputs(R, mirror, "%s, %s, kind %d" % (what, stage, kind))
            assert R.nsingular == (oc.nsingular_of(ob, D.basis, data, mirror[3]) if D else 0), (what, stage, kind)
            if not D:
                raw.append(R)
    return raw


def highpass_raw_and_detrended(E, ob, ncomp, niter, what):
    """highpass_observed on the raw data and on the residuals of detrend_observed(ncomp, niter), halves 5 and 70 under a
    boxcar, a Gaussian and a random table: the mirror's bits and ndead"""
    for stage in ("raw", "detrended"):
        data = E.detrend_observed(ncomp, niter).data if stage == "detrended" else ob.data
        for half in (5, 70):
            for name, hp in hc.tables(half).items():
                want, ndead = xcor.highpass_observed_reference(data, ob.weight, ob.seg_first, hp)
                E.set_highpass(hp)
                R = E.highpass_observed()
                assert same_bits(R.data, want) and R.ndead == ndead == np.count_nonzero(ob.weight == 0), (what, stage, half, name)
    E.set_highpass(None)


def normalise_both_recipes(E, ob, what):
    for nm in oc.RECIPES:
        E.set_normalise(nm)
        N = E.normalise_observed()
        oc.check_normalised(N, xcor.normalise_reference(ob.data, ob.weight, ob.seg_first, nm), "%s, %s" % (what, nc.name(nm)))
        assert np.isfinite(N.data).all()
    E.set_normalise(None)


@pytest.mark.parametrize("nexp", mc.NEXPS)
def test_weigh_observed(case, nexp):
    ms, px, ob = case.exposures(nexp)
    E = case.handle(px, ob)
    weigh_raw_and_detrended(E, ob, 3, 2, ms.name)
    E.close()


@pytest.mark.parametrize("nexp", mc.NEXPS)
def test_highpass_observed(case, nexp):
    ms, px, ob = case.exposures(nexp)
    E = case.handle(px, ob)
    highpass_raw_and_detrended(E, ob, 3, 2, ms.name)
    E.close()


@pytest.mark.parametrize("nexp", mc.NEXPS)
def test_normalise_observed(case, nexp):
    ms, px, ob = case.exposures(nexp)
    E = case.handle(px, ob)
    normalise_both_recipes(E, ob, ms.name)
    E.close()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ncomp", [5, 16])
@pytest.mark.parametrize("nexp", [64, 65])
def test_pca(case, nexp, ncomp, weighted):
    """with 5 % masked entries only 3 to 4 % of the columns are whole at these exposure counts: a segment without one has
    nwhole 0 and a zero basis"""
    ms, px, full = case.exposures(nexp)
    ob = full if weighted else ms.observed(case.scale, weighted=False)
    E = case.handle(px, ob)
    what = "%s, PCA of %d components, %s" % (ms.name, ncomp, "edge weights" if weighted else "no weights")
    mirror = xcor.pca_reference(ob.data, ob.weight, ob.seg_first, ncomp, 8)
    D = E.pca_observed(ncomp, 8)
    oc.check_pca_outputs(D, mirror, ob, what)
    nwhole = mirror[5]
    assert np.array_equal(D.nwhole, nwhole) and (weighted or np.array_equal(nwhole, ms.lengths)), what
    for s in range(ms.nseg):
        if nwhole[s] == 0:
            assert np.all(D.basis[s] == 0) and not np.signbit(D.basis[s]).any() and np.all(D.eigen[s] == 0), (what, s)
        else:
            assert np.any(D.basis[s, :, 0] != 0), (what, s)
    assert nwhole[5] == 0 and nwhole[7] > 0, what
    print("%s: the mirror's seven; nwhole %s, nsingular %d" % (what, D.nwhole, D.nsingular))
    E.close()


def test_pca_above_its_cap_is_refused(case):
    ms, px, ob = case.exposures(130)
    E = case.handle(px, ob)
    with pytest.raises(EngineError) as ei:
        E.pca_observed(5, 8)
    assert ei.value.code == -1 and "nexp 130 is above TRX_PCA_MAX_EXP (128)" in str(ei.value)
    E.close()


# ---- many orders ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg", mc.NSEGS)
def test_orders_moments_trail_and_velocity_map(case, nseg):
    ms, px, ob = case.orders(nseg)
    E = case.handle(px, ob)
    trail = oc.check_moments_and_trail(case, E, ms, ob)
    # the dead segment's statistic is undefined in the mirror and skipped on the device: per is finite all the same
    empty = np.flatnonzero(np.array(ms.lengths) == 0)
    for stat in ("ccf", "loglike_bl19"):
        st = ms.the_map(stat).statistic(trail)
        assert np.isnan(st[:, :, ms.dead_seg]).all() and np.isnan(st[:, :, empty]).all()
        assert np.isfinite(st[:, 0, 5]).all() and np.isnan(st[:, ms.masked_exp, ms.masked_seg]).all()
    got = oc.check_velocity_map(case, E, ms, trail)
    for stat in STATS:
        assert np.isfinite(got[stat][1]).all()
    E.close()


@pytest.mark.parametrize("nseg", mc.NSEGS)
def test_orders_filtered_map(case, nseg):
    oc.check_filtered_map(case, *case.orders(nseg), "plain %d" % mc.ORDERS_NCOMP)


@pytest.mark.parametrize("nseg", mc.NSEGS)
def test_orders_sysrem(case, nseg):
    ms, px, ob = case.orders(nseg)
    E = case.handle(px, ob)
    D = E.detrend_observed(mc.ORDERS_NCOMP, 10)
    oc.check_sysrem_outputs(D, xcor.sysrem_reference(ob.data, ob.weight, ob.seg_first, mc.ORDERS_NCOMP, 10), ob, ms.name)
    lengths = np.array(ms.lengths)
    empty = np.flatnonzero(lengths == 0)
    assert empty.min() < 64 and (nseg < 130 or empty.max() > 64)
    assert np.all(D.basis[empty] == 0) and not np.signbit(D.basis[empty]).any()
    assert np.all(D.basis[ms.dead_seg] == 0) and np.all(D.coef[:, ms.segment(ms.dead_seg)] == 0)
    live = np.flatnonzero(lengths > 0)
    live = live[live != ms.dead_seg]
    assert np.all(np.any(D.basis[live, :, 0] != 0, axis=1))
    assert D.nsingular >= 1 + lengths[ms.dead_seg]
    print("%s: basis, coef, data and nsingular (%d) are the mirror's" % (ms.name, D.nsingular))
    E.close()


def orders_edges(ms, nseg):
    """(the empty segments -- on both sides of index 64 where there is another side --, the dead segment's pixels)"""
    empty = np.flatnonzero(np.array(ms.lengths) == 0)
    assert empty.min() < 64 and (nseg < 130 or empty.max() > 64)
    return empty, ms.segment(ms.dead_seg)


@pytest.mark.parametrize("nseg", mc.NSEGS)
def test_orders_pca(case, nseg):
    ms, px, ob = case.orders(nseg)
    E = case.handle(px, ob)
    mirror = xcor.pca_reference(ob.data, ob.weight, ob.seg_first, mc.ORDERS_NCOMP, 8)
    D = E.pca_observed(mc.ORDERS_NCOMP, 8)
    oc.check_pca_outputs(D, mirror, ob, ms.name)
    empty, dead = orders_edges(ms, nseg)
    for s in list(empty) + [ms.dead_seg]:
        assert np.all(D.basis[s] == 0) and not np.signbit(D.basis[s]).any() and D.nwhole[s] == 0 and np.all(D.eigen[s] == 0) and D.offdiag[s] == 0, s
    assert np.all(D.coef[:, dead] == 0) and np.array_equal(D.data[:, dead], ob.data[:, dead])
    for s in np.flatnonzero(D.nwhole == 0):
        assert np.all(D.basis[s] == 0) and not np.signbit(D.basis[s]).any(), s
    assert np.count_nonzero(D.nwhole > 0) > nseg // 2 and np.all(np.any(D.basis[D.nwhole > 0][:, :, 0] != 0, axis=1))
    print("%s: the mirror's seven; %d segments with whole columns, nsingular %d" % (ms.name, np.count_nonzero(D.nwhole > 0), D.nsingular))
    E.close()


@pytest.mark.parametrize("nseg", mc.NSEGS)
def test_orders_weigh_observed(case, nseg):
    ms, px, ob = case.orders(nseg)
    E = case.handle(px, ob)
    raw = weigh_raw_and_detrended(E, ob, mc.ORDERS_NCOMP, 10, ms.name)
    empty, dead = orders_edges(ms, nseg)
    for R in raw:
        med = R.median[list(empty) + [ms.dead_seg]]
        assert np.all(med == 0) and not np.signbit(med).any()
        assert np.all(R.variance[dead] == 0) and np.all(R.weight[:, dead] == 0)
        live = np.delete(np.arange(nseg), list(empty) + [ms.dead_seg])
        assert np.count_nonzero(R.median[live] > 0) > nseg // 2
    E.close()


@pytest.mark.parametrize("nseg", mc.NSEGS)
def test_orders_highpass_observed(case, nseg):
    ms, px, ob = case.orders(nseg)
    E = case.handle(px, ob)
    highpass_raw_and_detrended(E, ob, mc.ORDERS_NCOMP, 10, ms.name)
    E.set_highpass(oc.HP)
    R = E.highpass_observed()
    empty, dead = orders_edges(ms, nseg)
    assert np.all(R.data[:, dead] == 0) and not np.signbit(R.data[:, dead]).any()      # dead entries are +0
    E.close()


@pytest.mark.parametrize("nseg", mc.NSEGS)
def test_orders_normalise_observed(case, nseg):
    """the two recipes, then detrend_observed and pca_observed at ORDERS_NCOMP with MEDIAN_RATIO installed"""
    ms, px, ob = case.orders(nseg)
    E = case.handle(px, ob)
    normalise_both_recipes(E, ob, ms.name)
    E.set_normalise(oc.MEDIAN_RATIO)
    norm = xcor.normalise_reference(ob.data, ob.weight, ob.seg_first, oc.MEDIAN_RATIO)
    empty, dead = orders_edges(ms, nseg)
    assert np.all(norm[1][:, list(empty) + [ms.dead_seg]] == 0) and np.all(norm[0][:, dead] == 0) and not np.signbit(norm[0][:, dead]).any()
    D = E.detrend_observed(mc.ORDERS_NCOMP, 10)
    oc.check_sysrem_outputs(D, xcor.sysrem_reference(norm[0], ob.weight, ob.seg_first, mc.ORDERS_NCOMP, 10), ob, ms.name)
    D = E.pca_observed(mc.ORDERS_NCOMP, 8)
    oc.check_pca_outputs(D, xcor.pca_reference(norm[0], ob.weight, ob.seg_first, mc.ORDERS_NCOMP, 8), ob, ms.name)
    E.close()


def test_orders_batch_of_two_ways(case):
    P = case.P
    ms, px, ob = case.orders(130)
    K = 3
    atms, keep = pc.atmospheres(P, K)
    vm = ms.the_map("loglike_bl19")
    one = case.handle(px, ob)
    ref = [one.run_velocity_map(atms[j], P.opts, vm, per=True) for j in range(K)]
    one.close()
    assert len({r[1].tobytes() for r in ref}) == K
    B = Batch(P.static, ways=2)
    B.set_pixels(px)
    B.set_observed(ob)
    m, per = B.run_velocity_map(atms, P.opts, vm, per=True)
    assert m.shape == (K, 3, 4) and per.shape == (K, LAGS.size, ms.nexp)
    for j in range(K):
        assert same_bits(m[j], ref[j][0]) and same_bits(per[j], ref[j][1]), j
    B.close()
