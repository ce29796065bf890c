"""What the device tests of the observed-set products share -- SYSREM, PCA, regression, normalisation, scatter weights, the
data-side high-pass, and the same products past 64 exposures, past 64 segments and at detector-length orders: one Case over
one problem, the builder every module's `case` fixture calls, and the checks of a call's outputs against its mirror in
transit_amd.xcor, all BIT FOR BIT.  A plain module: pytest collects nothing here and rewrites no assert, so every assert
below carries what it compared.

The problem is pixel_cases.make("eclipse", 20 000 lines, 6001 bins), the pixels xcor_checks.pixel_set's 800 with their two
off-grid ones, the segments [1, 63, 64, 65, 200, 0, 7, 400].  Every module builds its own problem and its own handles: what
is shared here is code, not state."""
import numpy as np

import hpdata_cases as hc
import many_cases as mc
import pixel_cases as pc
import scatter_cases as cs
import sysrem_cases as sc
import wfilter_cases as wc
import xcor_checks as xc
from bits import first_difference, same_bits
from transit_amd import pixels, xcor
from transit_amd.engine import Engine


# ---- the case of the 800 pixels -------------------------------------------------------------------------------------
class Case:
    """the problem, its pixel set, its spectrum and the spectrum's mean, and -- made once, on first use -- the raw observed
    sets a subclass's make_observed builds and whatever mirrors of them a test asks to keep"""

    def __init__(self, P, px, scale, spec):
        self.P, self.px, self.scale, self.spec = P, px, scale, spec
        self.sets, self.mirrors = {}, {}

    def make_observed(self, nexp, weighted):
        raise NotImplementedError("the subclass's observed set")

    def observed(self, nexp=7, weighted=True, *more):
        """the raw observed set, made once"""
        key = (nexp, weighted) + more
        if key not in self.sets:
            self.sets[key] = self.make_observed(*key)
        return self.sets[key]

    def memo(self, key, make):
        """make() of a mirror, once per key"""
        if key not in self.mirrors:
            self.mirrors[key] = make()
        return self.mirrors[key]

    def gain(self, nexp):
        return np.random.default_rng(60 + nexp).uniform(0.5, 1.5, sc.NPIX)

    def handle(self, ob, px=None, hp=None):
        E = Engine(self.P.static)
        E.set_pixels(self.px if px is None else px)
        if ob is not None:
            E.set_observed(ob)
        if hp is not None:
            E.set_highpass(hp)
        return E


class SysremCase(Case):
    """sysrem_cases' set at the model's scale: smooth trends plus seeded noise, the edge weights"""

    def make_observed(self, nexp, weighted):
        w = sc.edge_weights(nexp, 80 + nexp) if weighted else None
        return xcor.Observed(sc.SEG, self.scale * sc.data_set(nexp, 70 + nexp), w, self.gain(nexp))


class ScatterCase(Case):
    """scatter_cases.the_set at the model's scale: faint trends plus seeded noise with the planted columns"""

    def make_observed(self, nexp, weighted, seg=cs.SEG):
        data, w, _ = cs.the_set(nexp, weighted, self.scale)
        return xcor.Observed(seg, data, w, self.gain(nexp))


def build_case(tmp, cls):
    """what every module's `case` fixture does: the eclipse problem of 20 000 lines in the directory tmp, the 800 pixels, one
    run for the spectrum and its mean"""
    P = pc.make(tmp, "eclipse", nlines=20_000)
    px = xc.pixel_set(P)
    assert sc.LENGTHS == xc.LENGTHS and len(px) == sc.NPIX, (sc.LENGTHS, xc.LENGTHS, len(px), sc.NPIX)
    E = Engine(P.static)
    spec = E.run(P.atm, P.opts)["spectrum"]
    E.close()
    return cls(P, px, float(np.mean(spec)), spec)


# ---- a call's outputs against its mirror ----------------------------------------------------------------------------
def nsingular_of(ob, basis, data=None, weight=None):
    """the dead columns of the weighted filter of `basis` over ob's weights -- or, where a call has replaced them, over
    `data` and `weight` --: the mirror of the install step"""
    if data is not None or weight is not None:
        ob = xcor.Observed(ob.seg_first, data, weight, ob.gain)
    return int(np.count_nonzero(~xcor.weighted_factor(ob, xcor.WeightedFilter(basis))[2]))


def same_detrend(a, b):
    return same_bits(a.basis, b.basis) and same_bits(a.coef, b.coef) and same_bits(a.data, b.data) and a.nsingular == b.nsingular


def check_sysrem_outputs(D, mirror, ob, what):
    basis, coef, resid = mirror
    assert np.isfinite(basis).all() and np.isfinite(resid).all(), (what, "the mirror is not finite")
    assert same_bits(D.basis, basis), (what, "basis", first_difference(D.basis, basis))
    assert same_bits(D.coef, coef), (what, "coef", first_difference(D.coef, coef))
    assert same_bits(D.data, resid), (what, "data", first_difference(D.data, resid))
    assert D.nsingular == nsingular_of(ob, basis), (what, D.nsingular, nsingular_of(ob, basis))


def check_pca_outputs(D, mirror, ob, what):
    basis, coef, resid, eigen, offdiag, nwhole = mirror
    assert np.isfinite(basis).all() and np.isfinite(resid).all(), (what, "the mirror is not finite")
    assert same_bits(D.basis, basis), (what, "basis", first_difference(D.basis, basis))
    assert same_bits(D.coef, coef), (what, "coef", first_difference(D.coef, coef))
    assert same_bits(D.data, resid), (what, "data", first_difference(D.data, resid))
    assert same_bits(D.eigen, eigen), (what, "eigen", first_difference(D.eigen, eigen))
    assert same_bits(D.offdiag, offdiag), (what, "offdiag", first_difference(D.offdiag, offdiag))
    assert D.nwhole.dtype == np.int64 and np.array_equal(D.nwhole, nwhole), (what, D.nwhole.dtype, D.nwhole.tolist(), np.asarray(nwhole).tolist())
    assert D.nsingular == nsingular_of(ob, basis), (what, D.nsingular, nsingular_of(ob, basis))


def check_scatter_outputs(R, mirror, what):
    var, med, keep, w = mirror
    assert same_bits(R.variance, var), (what, "variance", first_difference(R.variance, var))
    assert same_bits(R.median, med), (what, "median", first_difference(R.median, med))
    assert same_bits(R.weight, w), (what, "weight", first_difference(R.weight, w))
    assert R.nmasked == np.count_nonzero((var > 0) & ~keep), (what, R.nmasked, np.count_nonzero((var > 0) & ~keep))


MEDIAN_RATIO = xcor.Normalise(xcor.NORM_ROW_QUANTILE, xcor.NORM_COL_RATIO, 0.5, 0.0)


def check_normalised(N, mirror, what):
    data, scale, centre, nclipped, nbad = mirror
    assert same_bits(N.rowscale, scale), (what, "rowscale", first_difference(N.rowscale, scale))
    assert same_bits(N.centre, centre), (what, "centre", first_difference(N.centre, centre))
    assert same_bits(N.data, data), (what, "data", first_difference(N.data, data))
    assert (N.nclipped, N.nbad) == (nclipped, nbad), (what, (N.nclipped, N.nbad), (nclipped, nbad))


# ---- past 64 exposures, past 64 segments, and at detector-length orders -------------------------------------------------
HP = hc.tables(70)["gauss"]
RECIPES = [MEDIAN_RATIO, xcor.Normalise(xcor.NORM_ROW_QUANTILE, xcor.NORM_COL_DIVIDE, 0.9, 3.0)]
MANY_OUTSIDE = np.zeros((3, 4), dtype=bool)
MANY_OUTSIDE[mc.OUTSIDE_CELL] = True
MANY_INSIDE = [(int(i), int(j)) for i, j in np.argwhere(~MANY_OUTSIDE)]


class ManyCase:
    """the problem, its spectrum's scale, and -- made once, on first use -- the pixel set and the observed set of every set"""

    def __init__(self, P, scale, spec):
        self.P, self.scale, self.spec = P, scale, spec
        self.made = {}

    def exposures(self, nexp):
        """(set, pixels, observed set) of nexp exposures over xcor_checks.pixel_set's 800 pixels"""
        if ("exp", nexp) not in self.made:
            ms = mc.exposures_set(nexp)
            assert ms.lengths == xc.LENGTHS and ms.off_grid == xc.OFF_GRID, (ms.lengths, ms.off_grid)
            self.made["exp", nexp] = (ms, xc.pixel_set(self.P), ms.observed(self.scale))
        return self.made["exp", nexp]

    def orders(self, nseg):
        """(set, pixels, observed set) of nseg segments: pixels of pixel_cases' two kinds (R = 20 000 on the same centres
        as R = 3000, windows of a lane and of a wave), cut down to the set's, one of them off the grid"""
        if ("seg", nseg) not in self.made:
            ms = mc.orders_set(nseg)
            half = (ms.npix + 1) // 2
            centres = np.linspace(2503, 2557, half) + 0.37 * float(self.P.static.wn_d)
            both = pc.joined(pixels.resolving_power(centres, 20000.0, 4.0), pixels.resolving_power(centres, 3000.0, 4.0))
            px = pixels.Pixels(both.centre[:ms.npix].copy(), both.fwhm[:ms.npix].copy(), both.cut)
            for p, c in ms.off_grid.items():
                px.centre[p] = c
            self.made["seg", nseg] = (ms, px, ms.observed(self.scale))
        return self.made["seg", nseg]

    def handle(self, px, ob):
        E = Engine(self.P.static)
        E.set_pixels(px)
        E.set_observed(ob)
        return E


class Cells:
    """what xcor_checks.check_contract takes for a case: the observed set, the filter, the pairs at the lags, and the
    filtered moments of every distinct lag row a map's cells take, made once per handle"""

    def __init__(self, P, ob, F, pairs=None, pairs_lv=None):
        self.P, self.ob, self.F, self.pairs, self.pairs_lv = P, ob, F, pairs, pairs_lv
        self.moms, self.refs = {}, {}

    def moments(self, E, idx, key="plain"):
        k = (key, np.asarray(idx, dtype=np.int64).tobytes())
        if k not in self.moms:
            self.moms[k] = E.run_filtered_moments(self.P.atm, self.P.opts, mc.LAGS[idx])
        return self.moms[k]

    def rows(self, idx):
        """the pair rows [nexp, npix, 2] of a cell"""
        return self.pairs[idx] if self.pairs is not None else self.pairs_lv[idx, np.arange(self.ob.nexp)]

    def reference(self, idx):
        """(mom, D) of a cell by xcor_checks.row_bounds' docstring: numpy's moments and the most the device's may differ from
        them.  Behind a weighted filter the values are the mirror's bit for bit (test_weighted_filter asserts it), so the
        docstring's tau is 0 and only the moments' own rule is left in D"""
        k = np.asarray(idx, dtype=np.int64).tobytes()
        if k not in self.refs:
            if isinstance(self.F, xcor.WeightedFilter):
                val = xcor.weighted_filter_reference(self.rows(idx), self.ob, self.F)
                mom, S = xcor.reference_values(val, self.ob), xcor.abs_reference_values(val, self.ob)
                D = (int(np.max(np.diff(self.ob.seg_first))) + 16) * xc.EPS * S
                D[..., 0] = 0.0
                self.refs[k] = (mom, D)
            else:
                self.refs[k] = xc.moment_differences(self, self.rows(idx))
        return self.refs[k]


def check_moments_and_trail(case, E, ms, ob):
    """run_moments against the definition; run_trail bit for bit against run_moments at three lags and against the definition;
    returns the trail"""
    P = case.P
    pairs = E.run_pixels(P.atm, P.opts, ms.shifts)
    for p in ms.off_grid:
        assert np.all(pairs[:, p, 1] == 0), (ms.name, "off-grid pixel", p, pairs[:, p, 1].max())
    assert np.count_nonzero(pairs[..., 1] > 0) == ms.nexp * (ms.npix - len(ms.off_grid)), (ms.name, np.count_nonzero(pairs[..., 1] > 0), ms.nexp * (ms.npix - len(ms.off_grid)))
    mom = E.run_moments(P.atm, P.opts, ms.shifts)
    xc.check_moments(mom, pairs, ob, ms.name)
    rows = [mom[ms.masked_exp, ms.masked_seg]] + ([mom[:, ms.dead_seg]] if ms.dead_seg is not None else [])
    for row in rows:                                           # masked over the segment: seven +0, no sign bit
        assert np.all(row == 0) and not np.signbit(row).any(), (ms.name, "a masked row is not seven +0", row.tolist())
    others = np.delete(np.arange(ms.nexp), ms.masked_exp)
    assert np.all(mom[others, ms.masked_seg, 0] > 0), (ms.name, "counts of the masked segment at the other exposures", mom[others, ms.masked_seg, 0].min())
    trail = E.run_trail(P.atm, P.opts, mc.LAGS)
    assert trail.shape == (mc.LAGS.size, ms.nexp, ms.nseg, 7), (ms.name, trail.shape)
    for l in (0, mc.LAGS.size // 2, mc.LAGS.size - 1):
        assert np.array_equal(trail[l], E.run_moments(P.atm, P.opts, np.full(ms.nexp, mc.LAGS[l]))), (ms.name, l)
    xc.check_trail(trail, E.run_pixels(P.atm, P.opts, mc.LAGS), ob, "%s, %d lags" % (ms.name, mc.LAGS.size))
    return trail


def check_velocity_map(case, E, ms, trail):
    """per against trail_statistic of the trail (ccf and chi2 in bits), the map bit for bit map_from_per of that per, NaN in
    the one outside cell; returns {stat: (map, per)}"""
    P = case.P
    out = {}
    for stat in xc.STATS:
        vm = ms.the_map(stat)
        m, per = E.run_velocity_map(P.atm, P.opts, vm, per=True)
        want = xc.check_per(per, trail, vm, ms.name)
        if stat != "loglike_bl19":
            assert same_bits(per, want), (ms.name, stat, "per", first_difference(per, want))
        assert same_bits(m, xcor.map_from_per(per, vm)), (ms.name, stat, "map", first_difference(m, xcor.map_from_per(per, vm)))
        assert np.array_equal(np.isnan(m), MANY_OUTSIDE), (ms.name, stat, "NaN cells", np.argwhere(np.isnan(m)).tolist())
        out[stat] = (m, per)
    return out


def check_map(E, C, ms, vm, m, idx, what, key="plain"):
    """a per-cell map: every inside cell against cell_value of run_filtered_moments at its lags within cell_bound, and
    against numpy alone by the propagation of xcor_checks.row_bounds' docstring"""
    assert np.array_equal(idx, xcor.nearest_lags(vm)) and np.array_equal(np.isnan(m), MANY_OUTSIDE), (what, vm.stat, "lag indices or NaN cells", np.argwhere(np.isnan(m)).tolist())
    xc.check_contract(C, E, vm, m, idx, key=key, what=what)
    worst = 0.0
    for i, j in MANY_INSIDE:
        mom, D = C.reference(idx[i, j])
        ref = xcor.cell_value(mom, vm)
        rows, small = xc.row_bounds(mom, D, vm)
        assert small < 1e-3, (what, vm.stat, i, j, small)
        tol = 2.0 * float(np.sum(rows)) + xcor.cell_bound(mom, vm)
        assert tol > 0 and abs(m[i, j] - ref) <= tol, (what, vm.stat, i, j, m[i, j], ref, tol)
        worst = max(worst, abs(m[i, j] - ref) / tol)
    print("%s %s: worst |map - numpy| / tolerance %.3e over the %d inside cells" % (what, vm.stat, worst, len(MANY_INSIDE)))


def install(E, ob, which):
    """'plain N': xcor_checks.random_filter; 'weighted N': a weighted filter of wfilter_cases.random_basis, whose dead count is the
    mirror's"""
    kind, ncomp = which.split()
    if kind == "plain":
        F = xc.random_filter(ob.nseg, int(ncomp), ob.nexp, seed=20 + int(ncomp))
        E.set_filter(F)
    else:
        F = xcor.WeightedFilter(wc.random_basis(ob.nseg, ob.nexp, int(ncomp), seed=50 + int(ncomp)))
        dead = E.set_weighted_filter(F)
        assert dead == np.count_nonzero(~xcor.weighted_factor(ob, F)[2]), (which, dead, np.count_nonzero(~xcor.weighted_factor(ob, F)[2]))
    return F


def check_filtered_map(case, ms, px, ob, which):
    P = case.P
    E = case.handle(px, ob)
    F = install(E, ob, which)
    C = Cells(P, ob, F, pairs=E.run_pixels(P.atm, P.opts, mc.LAGS))
    for stat in xc.STATS:
        vm = ms.the_map(stat)
        m, idx = E.run_filtered_map(P.atm, P.opts, vm, lag_index=True)
        check_map(E, C, ms, vm, m, idx, "%s, %s, filtered map" % (ms.name, which))
        if stat == "ccf":                                      # the cells' references are the definition's own
            ref = xcor.filtered_map_reference(C.pairs, ob, F, vm)
            assert np.array_equal(np.isnan(ref), MANY_OUTSIDE) and all(ref[c] == xcor.cell_value(C.reference(idx[c])[0], vm) for c in MANY_INSIDE), (ms.name, which, ref.tolist())
    E.close()
