"""What the device tests of the cross-correlation chain share -- moments, trail, Kp-Vsys map, the plain and the weighted
filter, the per-cell maps, the model-side high-pass: the 800-pixel set and its observed set, the lag and velocity grids, the
exposure tables, and the checks against transit_amd.xcor, each with its tolerance.  A plain module: pytest collects
nothing here and rewrites no assert, so every assert below carries the values it compared.

The problem is pixel_cases.make (6001 bins, 60 layers), the pixel set its 800-pixel joined set A + B (windows of 42-44 and
of 283-290 bins: both forms of the pair kernel) with two pixels (one in A, one in B) moved off the grid, to 2400 and
2700 cm-1: their pairs have b = 0 and count in no moment.  Segment lengths [1, 63, 64, 65, 200, 0, 7, 400]: one lane, a wave
less one, a wave, a wave plus one, several strides, an empty segment, a short one, the longest.

The tolerances, all derived, none measured.
Moments and trail rows (check_moments, check_trail, check_filtered_moments, check_weighted_moments), per moment, relative
to the same sum over |terms|: (n_max + 16) * 2^-52 with n_max the longest segment -- the worst case of a double sum of n
terms, (n - 1) * 2^-53 each way it is ordered, with each term made of at most four correctly rounded operations (a / b,
gain *, w *, * g), 4 * 2^-53 more, rounded up generously; the count is exact.  Behind a filter the sums are taken over the
VALUES THE DEVICE RETURNED, so that the cancellation inside g' does not enter.
Filtered values (check_values), per element, relative to xcor.filter_abs_reference A = |g| + |back| (|fwd| |g|):
(nexp + ncomp + 8) * 2^-52 -- two roundings in g, nexp products and sums in a coefficient, ncomp in the projection, one
subtraction, doubled to leave room for the reference's own rounding.
The statistic per lag and exposure (check_per) and a cell of a per-cell map (check_contract): xcor.per_bound and
xcor.cell_bound, derived in their docstrings.  A per-cell map against numpy alone: row_bounds, derived in its docstring."""
import numpy as np

import pixel_cases as pc
from transit_amd import _abi, pixels, xcor
from transit_amd.engine import Engine


# ---- the pixel set, the observed set and the moments --------------------------------------------------------------------
LENGTHS = [1, 63, 64, 65, 200, 0, 7, 400]
OFF_GRID = {250: 2400.0, 700: 2700.0}          # pixel -> centre (cm-1): one of set A, one of set B
EPS = 2.0 ** -52


def pixel_set(P):
    px = pc.joined(pc.set_a(P), pc.set_b(P))
    assert len(px) == 800 == sum(LENGTHS), (len(px), sum(LENGTHS))
    for p, c in OFF_GRID.items():
        px.centre[p] = c
    return px


def observed(npix, scale, lengths=LENGTHS, nexp=len(pc.SHIFTS), seed=3):
    """data around the model's scale, less their mean (so that sum w f g has both signs), weights in [0.5, 2] with
    5 % exact zeros, gains in [0.5, 1.5]"""
    rng = np.random.default_rng(seed)
    f = scale * (1.0 + 0.1 * rng.standard_normal((nexp, npix)))
    f -= f.mean()
    w = rng.uniform(0.5, 2.0, (nexp, npix))
    w[rng.random((nexp, npix)) < 0.05] = 0.0
    return xcor.Observed(xcor.segments(lengths), f, w, rng.uniform(0.5, 1.5, npix))


def check_moments(mom, pairs, ob, what=""):
    """the count exactly, every other moment to (n_max + 16) * 2^-52 of the sum of its absolute terms; an empty row is
    seven +0"""
    ref, scale = xcor.reference(pairs, ob), xcor.abs_reference(pairs, ob)
    assert mom.shape == ref.shape == (ob.nexp, ob.nseg, 7), (what, mom.shape, ref.shape)
    assert np.array_equal(mom[..., 0], ref[..., 0]), (what, "counts", np.argwhere(mom[..., 0] != ref[..., 0])[:4].tolist())
    n_max = int(np.max(np.diff(ob.seg_first)))
    tol = (n_max + 16) * EPS
    empty = ref[..., 0] == 0
    assert np.all(mom[empty] == 0) and not np.any(np.signbit(mom[empty])), (what, "an empty row is not seven +0", mom[empty][:2].tolist())
    err = np.abs(mom - ref)[~empty][:, 1:]
    ratio = err / scale[~empty][:, 1:]
    worst = float(ratio.max())
    print("%s: worst |mom - ref| / abs_ref %.3e = %.2f * 2^-52 (tolerance %.3e)" % (what, worst, worst / EPS, tol))
    assert worst <= tol, (what, worst, tol)
    return ref


# ---- the trail, and the planet of the end-to-end map --------------------------------------------------------------------
NEXP = len(pc.SHIFTS)
KP_TRUE, VSYS_TRUE = 100.0, 6.0
PHASE = np.linspace(-0.06, 0.06, NEXP)
TRAIL_KP, TRAIL_VSYS = np.array([40.0, 70.0, 100.0, 130.0, 160.0]), np.array([-12.0, -6.0, 0.0, 6.0, 12.0])
LAG_STEP = 3.0


def check_trail(trail, pairs, ob, what=""):
    """the count exactly, every other moment to (n_max + 16) * 2^-52 of the sum of its absolute terms; an empty row is
    seven +0"""
    ref, scale = xcor.trail_reference(pairs, ob), xcor.trail_abs_reference(pairs, ob)
    assert trail.shape == ref.shape == (pairs.shape[0], ob.nexp, ob.nseg, 7), (what, trail.shape, ref.shape)
    assert np.array_equal(trail[..., 0], ref[..., 0]), (what, "counts", np.argwhere(trail[..., 0] != ref[..., 0])[:4].tolist())
    tol = (int(np.max(np.diff(ob.seg_first))) + 16) * EPS
    empty = ref[..., 0] == 0
    assert np.all(trail[empty] == 0) and not np.any(np.signbit(trail[empty])), (what, "an empty row is not seven +0", trail[empty][:2].tolist())
    ratio = np.abs(trail - ref)[~empty][:, 1:] / scale[~empty][:, 1:]
    worst = float(ratio.max())
    print("%s: worst |trail - ref| / abs_ref %.3e = %.2f * 2^-52 (tolerance %.3e)" % (what, worst, worst / EPS, tol))
    assert worst <= tol, (what, worst, tol)
    return ref


def handle(P, px, ob):
    E = Engine(P.static)
    E.set_pixels(px)
    E.set_observed(ob)
    return E


def end_to_end_map(px, run_pixels, trail_of):
    """(map [5, 5], the injected cell): the data are the model's own pixel values at the planet's shifts times the gain,
    unit weights, two segments (the pixels at R = 20 000 and those at R = 3000); run_pixels(shifts) gives the pairs,
    trail_of(lags, ob) the trail of the observed set"""
    sin = np.sin(2 * np.pi * PHASE)
    with np.errstate(invalid="ignore", divide="ignore"):
        value = pixels.value(run_pixels(np.array([pixels.shift(v) for v in VSYS_TRUE + KP_TRUE * sin])))
    gain = np.random.default_rng(4).uniform(0.5, 1.5, len(px))
    data = np.where(np.isfinite(value), gain[None, :] * value, 0.0)           # (the off-grid pixels: any finite datum)
    ob = xcor.Observed(xcor.segments([400, 400]), data, None, gain)
    # the lag step is at most a quarter of the narrowest pixel's FWHM in velocity
    assert LAG_STEP <= 0.25 * pixels.C_KMS * float(np.min(px.fwhm / px.centre)), (LAG_STEP, 0.25 * pixels.C_KMS * float(np.min(px.fwhm / px.centre)))
    lag_kms, lags = xcor.lag_grid(-81.0, 81.0, LAG_STEP)
    assert lag_kms.size == 55, lag_kms.size
    trail = trail_of(lags, ob)
    assert trail.shape == (55, NEXP, 2, 7), trail.shape
    vp = TRAIL_VSYS[None, :, None] + TRAIL_KP[:, None, None] * sin[None, None, :]
    m = xcor.velocity_map(trail, lag_kms, vp, stat=xcor.ccf)
    assert m.shape == (5, 5) and np.all(np.isfinite(m)), m
    return m, (int(np.argmin(np.abs(TRAIL_KP - KP_TRUE))), int(np.argmin(np.abs(TRAIL_VSYS - VSYS_TRUE))))


# ---- the Kp-Vsys map: 55 lags, 7 x 5 and 13 x 11 cells ------------------------------------------------------------------
STATS = ("ccf", "loglike_bl19", "chi2")
ORBIT = np.sin(2 * np.pi * PHASE)
LAG_KMS, LAGS = xcor.lag_grid(-81.0, 81.0, LAG_STEP)
KP, VSYS = np.array([40.0, 70.0, 100.0, 130.0, 160.0, 190.0, 250.0]), np.arange(-12.0, 13.0, 6.0)
KP2, VSYS2 = np.linspace(30.0, 210.0, 13), np.linspace(-15.0, 15.0, 11)
OFFSET = 0.3 * np.cos(np.arange(len(PHASE)))
OUTSIDE = np.zeros((7, 5), dtype=bool)
OUTSIDE[6], OUTSIDE[5, [0, 4]] = True, True


def the_map(stat="ccf", second=False, offset=False, **over):
    kw = dict(lag_kms=LAG_KMS, kp=KP2 if second else KP, vsys=VSYS2 if second else VSYS, orbit=ORBIT,
              offset=OFFSET if offset is True else None if offset is False else offset,
              stat=stat, scale=0.9, a=1.1, b=0.2)
    kw.update(over)
    return xcor.VelocityMap(**kw)


def check_per(per, trail, vm, what):
    """per against trail_statistic of the trail within per_bound; the count of differing rows and the worst ratio"""
    want, tol = xcor.trail_statistic(trail, vm), xcor.per_bound(trail, vm)
    assert per.shape == want.shape and np.all(np.isfinite(per)) and np.all(tol > 0), (what, vm.stat, per.shape, want.shape, np.count_nonzero(~np.isfinite(per)), float(np.min(tol)))
    ratio = float(np.max(np.abs(per - want) / tol))
    print("%s %s: %d of %d rows differ from numpy, worst |per - ref| / per_bound %.4f" % (what, vm.stat, np.count_nonzero(per != want), per.size, ratio))
    assert ratio <= 1.0, (what, vm.stat, ratio)
    return want


# ---- the plain filter ---------------------------------------------------------------------------------------------------
STRADDLE = {100: 2561.0}                        # pixel (of set A) -> centre (cm-1): on the grid at the first shift only
DEAD = sorted(list(OFF_GRID) + list(STRADDLE))


def straddle_pixel_set(P, straddle=True):
    px = pixel_set(P)
    if straddle:
        for p, c in STRADDLE.items():
            px.centre[p] = c
    return px


def random_filter(nseg, ncomp, nexp, seed):
    """matrices of both signs, scaled to 1 / nexp"""
    rng = np.random.default_rng(seed)
    return xcor.Filter(rng.uniform(-1.0, 1.0, (nseg, ncomp, nexp)) / nexp, rng.uniform(-1.0, 1.0, (nseg, nexp, ncomp)) / nexp)


def check_values(val, pairs, ob, F, what=""):
    """NaN exactly where the definition has it, every other value to (nexp + ncomp + 8) * 2^-52 of A"""
    ref, scale = xcor.filter_reference(pairs, ob, F), xcor.filter_abs_reference(pairs, ob, F)
    assert val.shape == ref.shape == (ob.nexp, ob.npix), (what, val.shape, ref.shape)
    dead = np.isnan(ref)
    assert np.array_equal(np.isnan(val), dead), (what, "NaN pattern", np.argwhere(np.isnan(val) != dead)[:4].tolist())
    tol = (ob.nexp + F.ncomp + 8) * EPS
    err, size = np.abs(val - ref)[~dead], scale[~dead]
    worst = float(np.max(err[size > 0] / size[size > 0]))
    print("%s: worst |value - ref| / A %.3e = %.2f * 2^-52 (tolerance %.3e)" % (what, worst, worst / EPS, tol))
    assert np.all(err <= tol * size), (what, worst, tol)
    return ref


def check_filtered_moments(mom, val, ob, what=""):
    """the count exactly, every other moment to (n_max + 16) * 2^-52 of the sum of its absolute terms over the values
    the device returned; an empty row is seven +0"""
    ref, scale = xcor.reference_values(val, ob), xcor.abs_reference_values(val, ob)
    assert mom.shape == ref.shape == (ob.nexp, ob.nseg, 7), (what, mom.shape, ref.shape)
    assert np.array_equal(mom[..., 0], ref[..., 0]), (what, "counts", np.argwhere(mom[..., 0] != ref[..., 0])[:4].tolist())
    w = ob.weight if ob.weight is not None else np.ones_like(ob.data)
    full = np.diff(ob.seg_first) > 0
    want_n = np.add.reduceat((~np.isnan(val) & (w > 0)).astype(float), ob.seg_first[:-1][full], axis=1)
    assert np.array_equal(mom[..., 0][:, full], want_n), (what, "counts of the live values", np.argwhere(mom[..., 0][:, full] != want_n)[:4].tolist())
    tol = (int(np.max(np.diff(ob.seg_first))) + 16) * EPS
    empty = ref[..., 0] == 0
    assert np.all(mom[empty] == 0) and not np.any(np.signbit(mom[empty])), (what, "an empty row is not seven +0", mom[empty][:2].tolist())
    ratio = np.abs(mom - ref)[~empty][:, 1:] / scale[~empty][:, 1:]
    worst = float(ratio.max())
    print("%s: worst |mom - ref| / abs_ref %.3e = %.2f * 2^-52 (tolerance %.3e)" % (what, worst, worst / EPS, tol))
    assert worst <= tol, (what, worst, tol)


# ---- the per-cell maps --------------------------------------------------------------------------------------------------
CHUNK = _abi.CELLMAP_CHUNK
PIXEL = 100                                      # of set A, in segment 2
LIVE_UP_TO = 30.0                                # km/s: the last lag at which PIXEL's window is on the grid


def second_axes():
    """the 13 x 11 grid KP2 x VSYS2 -- with more Kp rows, should 143 cells not span three chunks with a ragged
    last one"""
    n = KP2.size
    while n * VSYS2.size <= 2 * CHUNK or (n * VSYS2.size) % CHUNK == 0:
        n += 1
    return (KP2 if n == KP2.size else np.linspace(30.0, 210.0, n)), VSYS2


FMAP_KP2, FMAP_VSYS2 = second_axes()


def the_filtered_map(stat="ccf", second=False, offset=False, **over):
    kw = dict(kp=FMAP_KP2, vsys=FMAP_VSYS2) if second else {}
    kw.update(over)
    return the_map(stat, second, offset, **kw)


def check_contract(case, E, vm, m, idx, key="plain", cells=None, what=""):
    """every inside cell (or the cells given) of m against cell_value of run_filtered_moments at its lags, within
    cell_bound; returns the number of cells that differ in bits"""
    differ, worst, n = 0, 0.0, 0
    for i, j in (cells if cells is not None else np.argwhere(np.all(idx >= 0, axis=-1))):
        mom = case.moments(E, idx[i, j], key)
        want, bound = xcor.cell_value(mom, vm), xcor.cell_bound(mom, vm)
        assert np.isfinite(m[i, j]) and bound > 0, (what, vm.stat, i, j)
        assert abs(m[i, j] - want) <= bound, (what, vm.stat, i, j, m[i, j], want, bound)
        differ += m[i, j] != want
        worst = max(worst, abs(m[i, j] - want) / bound)
        n += 1
    print("%s %s: %d of %d cells differ in bits from cell_value(run_filtered_moments), worst |map - ref| / cell_bound %.4f" % (what, vm.stat, differ, n, worst))
    return differ


def row_bounds(mom, D, vm):
    """[nexp, nseg]: the first-order bound of the statistic of every row (0 for a row the statistic skips), and the largest
    relative change of a variance or of the logarithm's argument it rests on.  For a per-cell map against numpy alone; nothing
    in it is measured.
      - values: the device's g' lies within tau * A of filter_reference's, tau = (nexp + ncomp + 8) 2^-52 and
        A = xcor.filter_abs_reference (check_values' rule), with NaN in the same columns;
      - moments (moment_differences): the exact sums over two value matrices that differ by at most tau A per element differ
        by at most E2 = sum w tau A in m2, E5 = sum w |f| tau A in m5 and E3 = sum w (2 |g'| tau A + (tau A)^2) in m3; m1, m4
        and m6 do not contain g.  On top of that each side's sum is not exact: the device's moments lie within
        (n_max + 16) 2^-52 of the sums S_k of their absolute terms (check_filtered_moments' rule, which leaves room for the
        reference's fsum), so moment k of the two sides differs by at most D_k = E_k + (n_max + 16) 2^-52 S_k; the count m0
        is exact;
      - the statistic of a row, to first order in the D_k, by the triangle inequality over its definition (s = m1):
            d<f> = (D4 + |<f>| D1) / s                       d<g> = (D2 + |<g>| D1) / s
            dsf2 = (D6 + (m6 / s) D1) / s + 2 |<f>| d<f>     dsg2 = (D3 + (m3 / s) D1) / s + 2 |<g>| d<g>
            dR   = (D5 + |m5 / s| D1) / s + |<f>| d<g> + |<g>| d<f>
            ccf           dR / sqrt(sf2 sg2) + (|ccf| / 2) (dsf2 / sf2 + dsg2 / sg2)
            loglike_bl19  (n / 2) (dsf2 + 2 |p0| dR + p0^2 dsg2) / arg
            chi2          D6 + 2 |p0| D5 + 2 |p1| D4 + p0^2 D3 + 2 |p0 p1| D2 + p1^2 D1          (exact: it is linear)
        doubled by the caller for the terms of second order, which needs the relative changes dsf2 / sf2, dsg2 / sg2 and
        d(arg) / arg to be small: the caller asserts that they are below 1e-3;
      - the cell: the sum of its rows' bounds, plus xcor.cell_bound of the reference's moments for the two evaluations of
        points 5 themselves."""
    p0, p1 = vm.params
    if vm.stat == "chi2":
        return D[..., 6] + 2 * abs(p0) * D[..., 5] + 2 * abs(p1) * D[..., 4] + p0 * p0 * D[..., 3] + 2 * abs(p0 * p1) * D[..., 2] + p1 * p1 * D[..., 1], 0.0
    n, sf2, sg2, r, ok = xcor.central(mom)
    with np.errstate(all="ignore"):
        s = mom[..., 1]
        mf, mg = mom[..., 4] / s, mom[..., 2] / s
        dmf, dmg = (D[..., 4] + np.abs(mf) * D[..., 1]) / s, (D[..., 2] + np.abs(mg) * D[..., 1]) / s
        dsf2 = (D[..., 6] + mom[..., 6] / s * D[..., 1]) / s + 2 * np.abs(mf) * dmf
        dsg2 = (D[..., 3] + mom[..., 3] / s * D[..., 1]) / s + 2 * np.abs(mg) * dmg
        dr = (D[..., 5] + np.abs(mom[..., 5] / s) * D[..., 1]) / s + np.abs(mf) * dmg + np.abs(mg) * dmf
        small = np.maximum(dsf2 / sf2, dsg2 / sg2)
        if vm.stat == "ccf":
            b = dr / np.sqrt(sf2 * sg2) + 0.5 * np.abs(r / np.sqrt(sf2 * sg2)) * (dsf2 / sf2 + dsg2 / sg2)
        else:
            arg = sf2 - 2 * p0 * r + p0 * p0 * sg2
            darg = dsf2 + 2 * abs(p0) * dr + p0 * p0 * dsg2
            ok = ok & (arg > 0)
            b = 0.5 * n * darg / arg
            small = np.maximum(small, darg / arg)
    return np.where(ok, b, 0.0), float(np.max(np.where(ok, small, 0.0)))


# ---- the weighted filter ------------------------------------------------------------------------------------------------
def check_weighted_moments(mom, val, ob, what=""):
    """check_filtered_moments' rule -- the count exactly, every other moment within (n_max + 16) * 2^-52 of the sum of its absolute
    terms over the values the device returned -- as an inequality, for rows whose sums of absolute terms are exact zeros
    (behind a high-pass the one pixel of a segment of one is g - g = 0) and for sets whose rows are all empty (9 components
    of 7 exposures: every column is dead)"""
    ref, scale = xcor.reference_values(val, ob), xcor.abs_reference_values(val, ob)
    assert mom.shape == ref.shape == (ob.nexp, ob.nseg, 7), (what, mom.shape, ref.shape)
    assert np.array_equal(mom[..., 0], ref[..., 0]), (what, "counts", np.argwhere(mom[..., 0] != ref[..., 0])[:4].tolist())
    tol = (int(np.max(np.diff(ob.seg_first))) + 16) * EPS
    empty = ref[..., 0] == 0
    assert np.all(mom[empty] == 0) and not np.any(np.signbit(mom[empty])), (what, "an empty row is not seven +0", mom[empty][:2].tolist())
    assert np.all(np.abs(mom - ref) <= tol * scale), (what, tol, np.argwhere(~(np.abs(mom - ref) <= tol * scale))[:4].tolist())
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(scale > 0, np.abs(mom - ref) / scale, 0.0)
    print("%s: worst |mom - ref| / abs_ref %.2f * 2^-52 (tolerance %.0f * 2^-52)" % (what, float(ratio.max()) / EPS, tol / EPS))


# ---- the model-side high-pass -------------------------------------------------------------------------------------------
def highpass_tables(half, seed=0):
    """a boxcar, a Gaussian and a random table (a fifth of its taps zero) of this half"""
    rng = np.random.default_rng(1000 + half + seed)
    rnd = np.concatenate([[0.7], rng.uniform(0.0, 2.0, half) * (rng.random(half) > 0.2)])
    gauss = np.exp(-(np.arange(half + 1.0) ** 2) / (2.0 * max(half / 3.0, 0.5) ** 2))
    return {"boxcar": xcor.boxcar_highpass(2 * half + 1), "gauss": xcor.HighPass(gauss), "random": xcor.HighPass(rnd)}


# ---- a cell's moments and their differences in numpy --------------------------------------------------------------------
def moment_differences(case, pr):
    """(mom, D) of a cell from its own pair rows pr [nexp, npix, 2], for row_bounds' propagation: the reference's moments
    [nexp, nseg, 7] and the most by which the device's can differ from them"""
    ob, F = case.ob, case.F
    val, A = xcor.filter_reference(pr, ob, F), xcor.filter_abs_reference(pr, ob, F)
    mom, S = xcor.reference_values(val, ob), xcor.abs_reference_values(val, ob)
    tA = (ob.nexp + F.ncomp + 8) * EPS * A
    lin = xcor.abs_reference_values(tA, ob)                       # sum w tA, sum w tA^2, sum w |f| tA
    cross = xcor.abs_reference_values(np.sqrt(np.abs(val) * tA), ob)      # sum w |g'| tA
    D = (int(np.max(np.diff(ob.seg_first))) + 16) * EPS * S
    D[..., 0] = 0.0
    D[..., 2] += lin[..., 2]
    D[..., 3] += 2.0 * cross[..., 3] + lin[..., 3]
    D[..., 5] += lin[..., 5]
    return mom, D


# ---- the exposure tables ------------------------------------------------------------------------------------------------
SMEAR = np.array([0.0, 2e-9, 1e-6, 3e-6, 1.3e-5, 0.0, 1e-5])         # exact 0 mixed with half-widths up to 1.3e-5 (7.8 km/s across the exposure)
SCALE = np.array([1.0, 0.5, 0.0, -0.25, 1.0, 3.0, 1e-3])             # the model-side tests' scales: 1, 0 and a negative value
SCALE0 = np.array([1.0, 0.5, 0.0, -0.25, 0.0, 3.0, 1e-3])            # the observed-set tests' scales: 0 at two exposures


# ---- a map small enough to follow by hand -------------------------------------------------------------------------------
def hand_case():
    """2 lags, 2 exposures, 2 segments of 2 pixels; lag 1's pixel 1 has no window on the grid.  The filter of segment 0 takes
    the mean over the two exposures out (fwd = (1/2, 1/2), back = (1, 1)); that of segment 1 takes exposure 0's value
    out of exposure 1 (fwd = (1, 0), back = (0, 1))."""
    g = np.array([[1.0, 2.0, 3.0, 4.0], [2.0, 9.0, 1.0, 5.0]])
    b = np.array([[1.0, 1.0, 1.0, 1.0], [1.0, 0.0, 1.0, 1.0]])
    pairs = np.stack([g * b, b], axis=-1)
    obs = xcor.Observed([0, 2, 4], [[1.0, 0.0, 2.0, 4.0], [0.0, 2.0, 1.0, 3.0]])
    filt = xcor.Filter([[[0.5, 0.5]], [[1.0, 0.0]]], [[[1.0], [1.0]], [[0.0], [1.0]]])
    return pairs, obs, filt
