"""The observed-set chain on the device at detector-length orders: moments, trail, Kp-Vsys map, plain and weighted filter, the
per-cell maps, SYSREM, PCA, the scatter weights, the data-side high-pass and the normalisation (include/transit_hip.h) against
transit_amd.xcor at many_cases.long_set -- 12 exposures of 1024, 1025, 0, 2049 and 7 pixels.

Every other device test of this chain borrows xcor_checks.pixel_set's 800 pixels, whose longest segment is 400 (736 in
hpdata_cases' "long" cut); the kernels have structure on the pixel axis that only shows at a detector's 2048:
  - k_scatter_median stages a segment's variances kScatLds = 1024 at a time: 1024 is one trip exactly, 1025 a second trip of
    one value padded to kScatTrip = 8 with +infinity, 2049 three trips; the ranks are carried from trip to trip, and the ties
    planted across trips leave med at 0 if they are miscounted.  The scatter tiles of 256 columns: four whole, four and one
    of ONE column, eight and one of one column;
  - the row reductions (k_pixel_moments, the trail, k_sysrem_rows, k_pca_gram, k_pca_live) take a segment 256 pixels a step:
    four whole steps, four and one lane, eight and one lane -- the mirrors reproduce the lane order;
  - k_data_highpass' tiles of kHpTile = 512: two whole, two and a tile of one pixel whose window is all halo, four and such a
    tile; a half of 600 reaches over more than two tiles;
  - k_norm_rowscale selects from a staging array of kNormCap = 2048 keys: 2049 is one above it.

No tolerance here is this file's own.  Every comparison is "the same bits" or one of the derived rules of the tests this file
borrows its checkers from, evaluated at the set's own nexp, ncomp and longest segment (2049): xcor_checks.check_moments
and xcor_checks.check_trail ((n_max + 16) * 2^-52 of the absolute sums), xcor_checks.check_per (xcor.per_bound),
xcor_checks.check_values and check_filtered_moments, xcor_checks.check_contract (xcor.cell_bound) and the propagation of
xcor_checks.row_bounds, observed_cases.check_sysrem_outputs, observed_cases.check_pca_outputs, observed_cases.check_scatter_outputs,
observed_cases.check_normalised and test_gpu_hpdata's rules (bits).  tests/test_many_cases_host.py holds the set's
preconditions; the *_host.py tests run the kernels' own source on the CPU over the same set against the same mirrors."""
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
from transit_amd import pixels, xcor
from transit_amd.engine import Engine

pytestmark = pytest.mark.gpu

V = xcor.SCATTER_VARIANCE
HALVES = mc.LONG_HALVES                                  # 0, 5, 70 and 600: more than kHpTile
HP, RECIPES = oc.HP, oc.RECIPES                          # the Gaussian table of half 70; MEDIAN_RATIO, and quantile 0.9 + divide + clip 3


class Case(oc.ManyCase):
    def long(self, weighted=True):
        """(set, planted, pixels, observed set): the long set whose ties are planted with or without the weights, the observed
        set with or without them; the pixel centres as test_gpu_normalise makes its edge set's, one of them off the grid"""
        if ("long", weighted) not in self.made:
            ms, pl = mc.long_set(weighted)
            px = pixels.resolving_power(np.linspace(2503.0, 2557.0, ms.npix), 20000.0, 4.0)
            for p, c in ms.off_grid.items():
                px.centre[p] = c
            self.made["long", weighted] = (ms, pl, px, ms.observed(self.scale, weighted=weighted))
        return self.made["long", weighted]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    P = pc.make(tmp_path_factory.mktemp("long"), "eclipse", nlines=20_000)
    E = Engine(P.static)
    spec = E.run(P.atm, P.opts)["spectrum"]
    E.close()
    return Case(P, float(np.mean(spec)), spec)


def long_of(case):
    ms, pl, px, ob = case.long()
    return ms, px, ob


# ---- moments, trail, maps and filters, through the borrowed checkers ------------------------------------------------
def test_moments_trail_and_velocity_map(case):
    ms, px, ob = long_of(case)
    E = case.handle(px, ob)
    trail = oc.check_moments_and_trail(case, E, ms, ob)
    got = oc.check_velocity_map(case, E, ms, trail)
    assert all(np.isfinite(got[stat][1]).all() for stat in xc.STATS)
    E.close()


@pytest.mark.parametrize("ncomp", [6, 16])
def test_plain_filter(case, ncomp):
    P = case.P
    ms, px, ob = long_of(case)
    E = case.handle(px, ob)
    F = xc.random_filter(ob.nseg, ncomp, ms.nexp, seed=ncomp)
    E.set_filter(F)
    what = "%s, plain filter of %d" % (ms.name, ncomp)
    pairs = E.run_pixels(P.atm, P.opts, ms.shifts)
    mom, val = E.run_filtered_moments(P.atm, P.opts, ms.shifts, values=True)
    xc.check_values(val, pairs, ob, F, what)
    assert np.flatnonzero(np.isnan(val).any(axis=0)).tolist() == sorted(ms.off_grid) and np.isnan(val[:, sorted(ms.off_grid)]).all()
    xc.check_filtered_moments(mom, val, ob, what)
    E.close()


def test_weighted_filter(case):
    P = case.P
    ms, px, ob = long_of(case)
    E = case.handle(px, ob)
    wf = xcor.WeightedFilter(wc.random_basis(ob.nseg, ms.nexp, 8, seed=58))
    live = xcor.weighted_factor(ob, wf)[2]
    assert E.set_weighted_filter(wf) == np.count_nonzero(~live) >= 1
    pairs = E.run_pixels(P.atm, P.opts, ms.shifts)
    mom, val = E.run_filtered_moments(P.atm, P.opts, ms.shifts, values=True)
    assert same_bits(val, xcor.weighted_filter_reference(pairs, ob, wf))
    dead = ~live
    dead[list(ms.off_grid)] = True
    assert np.array_equal(np.isnan(val).any(axis=0), dead) and np.isnan(val[:, dead]).all() and dead[ms.masked_col]
    assert np.count_nonzero(dead) < ms.npix // 4
    xc.check_weighted_moments(mom, val, ob, "%s, weighted filter of 8" % ms.name)
    E.close()


@pytest.mark.parametrize("which", ["plain 6", "plain 16", "weighted 8"])
def test_filtered_map(case, which):
    oc.check_filtered_map(case, *long_of(case), which)


# ---- SYSREM and PCA ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ncomp,niter", [(3, 10), (16, 10)])
def test_sysrem(case, ncomp, niter, weighted):
    ms, px, full = long_of(case)
    ob = full if weighted else ms.observed(case.scale, weighted=False)
    E = case.handle(px, ob)
    what = "%s, %d components of %d alternations, %s" % (ms.name, ncomp, niter, "edge weights" if weighted else "no weights")
    D = E.detrend_observed(ncomp, niter)
    oc.check_sysrem_outputs(D, xcor.sysrem_reference(ob.data, ob.weight, ob.seg_first, ncomp, niter), ob, what)
    assert np.all(D.basis[2] == 0) and not np.signbit(D.basis[2]).any() and np.all(np.any(D.basis[[0, 1, 3, 4], :, 0] != 0, axis=1)), what
    if weighted:
        row = D.basis[ms.masked_seg, ms.masked_exp]
        assert np.all(row == 0) and not np.signbit(row).any(), what
        assert np.array_equal(D.data[ms.masked_exp, ms.segment(ms.masked_seg)], ob.data[ms.masked_exp, ms.segment(ms.masked_seg)]), what
        assert np.all(D.coef[:, ms.masked_col] == 0) and D.nsingular >= 1, what
    print("%s: basis, coef, data and nsingular (%d) are the mirror's" % (what, D.nsingular))
    E.close()


def test_sysrem_with_injection(case):
    """8 components of 10 alternations with the model injected"""
    P = case.P
    ms, px, ob = long_of(case)
    E = case.handle(px, ob)
    pairs = E.run_pixels(P.atm, P.opts, ms.shifts)
    p0, p1 = 0.05 / case.scale, 0.9
    f0 = xcor.inject_reference(pairs, ob, p0, p1)
    on = pairs[..., 1] > 0
    assert np.count_nonzero(on) == ms.nexp * (ms.npix - 1) and np.all(f0[on] != ob.data[on])
    D = E.detrend_observed(8, 10, inject=(P.atm, P.opts, ms.shifts, p0, p1))
    oc.check_sysrem_outputs(D, xcor.sysrem_reference(f0, ob.weight, ob.seg_first, 8, 10), ob, "%s, injected" % ms.name)
    assert np.array_equal(D.spectrum, case.spec)
    E.close()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ncomp", [3, 5])
def test_pca(case, ncomp, weighted):
    ms, px, full = long_of(case)
    ob = full if weighted else ms.observed(case.scale, weighted=False)
    E = case.handle(px, ob)
    what = "%s, PCA of %d components, %s" % (ms.name, ncomp, "edge weights" if weighted else "no weights")
    D = E.pca_observed(ncomp, 8)
    oc.check_pca_outputs(D, xcor.pca_reference(ob.data, ob.weight, ob.seg_first, ncomp, 8), ob, what)
    assert np.all(D.basis[2] == 0) and not np.signbit(D.basis[2]).any() and D.nwhole[2] == 0, what
    for s in mc.LONG_SEGS:
        assert (0 < D.nwhole[s] < ms.lengths[s]) if weighted else (D.nwhole[s] == ms.lengths[s]), what
        assert np.all(np.any(D.basis[s] != 0, axis=0)), what
    if weighted:
        row = D.basis[ms.masked_seg, ms.masked_exp]
        assert np.all(row == 0) and not np.signbit(row).any(), what
    print("%s: the mirror's seven; nwhole %s, nsingular %d" % (what, D.nwhole, D.nsingular))
    E.close()


# ---- the scatter weights -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [True, False])
def test_weigh_observed(case, weighted):
    """raw and after detrend_observed(3, niter=2), test_gpu_scatter's stages.  The planted ties lie across staging trips: med of
    their segments is the pair's variance; at both stages a clip of 3 removes exactly the planted columns that are live, with
    no live column's var / med within 5 % of 9 (tests/test_many_cases_host.py holds both on the mirrors; after ten alternations
    SYSREM's components take some planted columns up, which is why the stage is niter = 2)."""
    ms, pl, px, ob = case.long(weighted)
    E = case.handle(px, ob)
    for stage in ("raw", "detrended"):
        D = E.detrend_observed(3, niter=2) if stage == "detrended" else None
        data = D.data if D else ob.data
        for kind in cs.KINDS:
            for clip in cs.CLIPS:
                for min_live in (2, ms.nexp):
                    what = "%s, %s, %s, kind %d, clip %g, min_live %d" % (ms.name, "edge weights" if weighted else "no weights", stage, kind, clip, min_live)
                    mirror = xcor.scatter_reference(data, ob.weight, ob.seg_first, kind, clip, min_live)
                    R = E.weigh_observed(kind, clip=clip, min_live=min_live)
                    oc.check_scatter_outputs(R, mirror, what)
                    assert R.nsingular == (oc.nsingular_of(ob, D.basis, data, mirror[3]) if D else 0), what
                    var, med, keep, _ = mirror
                    assert R.median[2] == 0 and not np.signbit(R.median[2]), what
                    if stage == "raw" and min_live == 2:
                        for s, a, b in pl.ties:
                            assert same_bits(R.median[s], var[a]) and same_bits(R.variance[a], R.variance[b]) and R.median[s] > 0, what
                    if clip:
                        clipped, margin = cs.clip_margin(var, med, keep, ob.seg_first)
                        print("%s: clipped %s, nearest var / (9 med) %.3f away from 1, nsingular %d" % (what, clipped, margin, R.nsingular))
                        got = tuple(int(p) for p in np.flatnonzero((R.variance > 0) & (R.weight.max(axis=0) == 0)))
                        assert got == clipped and margin > 0.05 and clipped == tuple(p for p in sorted(pl.noisy) if var[p] > 0), what
    E.close()


# ---- the data-side high-pass ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", ["raw", "residuals"])
def test_highpass_observed(case, stage):
    """on the raw data and on the device's own SYSREM residuals: every half under a boxcar, a Gaussian and a random table"""
    ms, px, ob = long_of(case)
    E = case.handle(px, ob)
    data = E.detrend_observed(3, 10).data if stage == "residuals" else ob.data
    for half in HALVES:
        for name, hp in hc.tables(half).items():
            what = "%s, %s, half %d, %s" % (ms.name, stage, half, name)
            want, ndead = xcor.highpass_observed_reference(data, ob.weight, ob.seg_first, hp)
            E.set_highpass(hp)
            R = E.highpass_observed()
            assert same_bits(R.data, want), what
            assert R.ndead == ndead == np.count_nonzero(ob.weight == 0), what
    E.close()


def test_highpass_two_kernels_one_definition(case):
    """test_gpu_hpdata.test_two_kernels_one_definition's rule, at a half above the tile length: the model's values installed as
    data, live where b > 0, give under the data kernel what the model kernel gives of the pairs themselves"""
    P = case.P
    ms, px, ob = long_of(case)
    Mo = case.handle(px, ob)
    pairs = Mo.run_pixels(P.atm, P.opts, ms.shifts)
    a, b = pairs[..., 0], pairs[..., 1]
    live = b > 0
    assert not live[:, list(ms.off_grid)].any() and np.count_nonzero(live.all(axis=0)) == ms.npix - 1
    with np.errstate(all="ignore"):
        g = np.where(live, ob.gain[None, :] * (a / np.where(live, b, 1.0)), 0.0)
    D = case.handle(px, xcor.Observed(ob.seg_first, g, live.astype(np.float64), None))
    hp = hc.tables(600)["random"]
    Mo.set_highpass(hp)
    D.set_highpass(hp)
    model = Mo.run_highpassed(P.atm, P.opts, ms.shifts)
    assert np.array_equal(np.isnan(model), ~live)
    R = D.highpass_observed()
    assert same_bits(R.data, np.where(live, model, 0.0))
    assert R.ndead == np.count_nonzero(~live)
    Mo.close()
    D.close()


# ---- the normalisation, and the detrending calls behind it ------------------------------------------------------------
@pytest.mark.parametrize("nm", RECIPES, ids=nc.name)
def test_normalise_then_detrend_and_pca(case, nm):
    ms, px, ob = long_of(case)
    E = case.handle(px, ob)
    what = "%s, %s" % (ms.name, nc.name(nm))
    E.set_normalise(nm)
    norm = xcor.normalise_reference(ob.data, ob.weight, ob.seg_first, nm)
    N = E.normalise_observed()
    oc.check_normalised(N, norm, what)
    assert np.isfinite(N.data).all() and N.rowscale[ms.masked_exp, ms.masked_seg] == 0 and np.all(N.rowscale[:, 2] == 0) and np.all(N.rowscale[:, 3] > 0), what
    basis, coef, resid = xcor.sysrem_reference(norm[0], ob.weight, ob.seg_first, 3, 10)
    D = E.detrend_observed(3, 10)
    oc.check_sysrem_outputs(D, (basis, coef, resid), ob, what)
    D = E.pca_observed(3, 8)
    oc.check_pca_outputs(D, xcor.pca_reference(norm[0], ob.weight, ob.seg_first, 3, 8), ob, what)
    E.set_normalise(None)
    assert not same_bits(E.detrend_observed(3, 10).data, resid)
    print("%s: %d entries clipped, %d bad; SYSREM and PCA of the normalised data are the mirrors'" % (what, N.nclipped, N.nbad))
    E.close()


# ---- the pipeline in order, on one handle ------------------------------------------------------------------------------
def test_the_pipeline_in_order_on_one_handle(case):
    """set_highpass, set_normalise, detrend_observed(5, 10, inject), highpass_observed, weigh_observed(VARIANCE, clip 3),
    run_filtered_map: each step against the mirror fed the previous mirror's output, the map against a fresh handle given the
    mirrors' data, weights and basis, and detrend_observed(0) back to the fresh handle's moments"""
    P = case.P
    ms, px, ob = long_of(case)
    E = case.handle(px, ob)
    pairs = E.run_pixels(P.atm, P.opts, ms.shifts)
    E.set_highpass(HP)
    E.set_normalise(oc.MEDIAN_RATIO)
    fresh = E.run_moments(P.atm, P.opts, ms.shifts)
    p0, p1 = 0.05 / case.scale, 0.9
    f0 = xcor.inject_reference(pairs, ob, p0, p1)
    norm = xcor.normalise_reference(f0, ob.weight, ob.seg_first, oc.MEDIAN_RATIO)[0]
    basis, coef, resid = xcor.sysrem_reference(norm, ob.weight, ob.seg_first, 5, 10)
    D = E.detrend_observed(5, 10, inject=(P.atm, P.opts, ms.shifts, p0, p1))
    oc.check_sysrem_outputs(D, (basis, coef, resid), ob, "the pipeline's detrend")
    hpd, ndead = xcor.highpass_observed_reference(resid, ob.weight, ob.seg_first, HP)
    H = E.highpass_observed()
    assert same_bits(H.data, hpd) and H.ndead == ndead
    mirror = xcor.scatter_reference(hpd, ob.weight, ob.seg_first, V, 3.0, 2)
    R = E.weigh_observed(V, clip=3.0)
    oc.check_scatter_outputs(R, mirror, "the pipeline's weigh")
    vm = ms.the_map("ccf")
    m, idx = E.run_filtered_map(P.atm, P.opts, vm, lag_index=True)
    assert np.array_equal(idx, xcor.nearest_lags(vm)) and np.array_equal(np.isnan(m), oc.MANY_OUTSIDE)
    F = case.handle(px, xcor.Observed(ob.seg_first, hpd, mirror[3], ob.gain))
    assert F.set_weighted_filter(xcor.WeightedFilter(basis)) == R.nsingular
    F.set_highpass(HP)
    want = F.run_filtered_map(P.atm, P.opts, vm)
    F.close()
    assert same_bits(m, want)
    print("the pipeline: %d entries dead, %d columns clipped, %d dead in the filter; the map is the fresh handle's" % (H.ndead, R.nmasked, R.nsingular))
    assert E.detrend_observed(0).nsingular == 0
    assert same_bits(E.run_moments(P.atm, P.opts, ms.shifts), fresh)
    E.close()
