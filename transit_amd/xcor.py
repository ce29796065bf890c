"""Host side of the moment runs, Engine.set_observed / Engine.run_moments and their Batch forms (trx_set_observed /
trx_run_moments, include/transit_hip.h): a high-resolution cross-correlation retrieval's comparison of the detector
pixels with the observed exposures, order by order, from seven weighted sums per (exposure, segment).

For exposure v and pixel p, (a, b) is the pixel run's pair, f the datum, w its weight (1 without weights).  A pixel
contributes when b > 0 and w > 0; its model value is g = gain_p * (a / b).  Over the contributing pixels of a segment

    mom[v, s] = (n, sum w, sum w g, sum w g^2, sum w f, sum w f g, sum w f^2)

    Observed(seg_first, data, weight=None, gain=None)    an observed set; to_c() its trx_observed
    segments(lengths)                                    seg_first from the segments' lengths
    reference(pairs, obs)                                the definition in numpy, sums by math.fsum
    abs_reference(pairs, obs)                            the same with |f| and |g|: the scale of a sum's rounding error
    chi2(mom, a=1, b=0)                                  sum w (f - a g - b)^2 per (v, s)
    ccf(mom)                                             the weighted Pearson coefficient of f and g per (v, s)
    loglike_bl19(mom, scale=1)                           the Brogi & Line (2019) log-likelihood per (v, s)
    chi2_sum, ccf_sum, loglike_bl19_sum                  the same added over all (v, s)

The trail (Engine.run_trail / Batch.run_trail; trx_run_trail): the same seven sums for every exposure against the model at
every lag of a velocity grid, trail[l, v, s] -- row l is the moments with lag l's pairs at all exposures.

    trail_reference(pairs, obs)                          the definition over the pairs [nlag, npix, 2] of run_pixels(lags)
    trail_abs_reference(pairs, obs)                      the same with |f| and |g|
    lag_grid(v_lo, v_hi, step)                           (lag_kms, lags): velocities v_lo, v_lo + step, ... and pixels.shift of each
    velocity_map(trail, lag_kms, v_planet, stat=ccf)     the statistic along each map cell's velocity track, added over exposures

The detection map on the device (Engine.run_velocity_map / Batch.run_velocity_map; trx_run_velocity_map): the trail
reduced there to per[l, v] = the statistic of the rows (l, v, .) added over the segments IN ORDER, and to the Kp-Vsys
map, per interpolated along each cell's velocity track and added over the exposures in order.

    VelocityMap(lag_kms, kp, vsys, orbit, offset=None, stat="ccf", scale=1, a=1, b=0)     a trx_vmap; to_c()
    trail_statistic(trail, vm)                           per [nlag, nexp]: the definition in numpy, segments added in order
    map_from_per(per, vm)                                the map [nkp, nvsys] from per: the definition in numpy
    map_reference(trail, vm)                             map_from_per(trail_statistic(trail, vm), vm)
    per_bound(trail, vm), map_bound(trail, vm)           how far two double evaluations of per / of a cell can lie apart

The detrending filter (Engine.set_filter / Engine.run_filtered_moments; trx_set_filter / trx_run_filtered_moments): per
segment s a coefficient matrix fwd[s] ([ncomp, nexp]) and a basis back[s] ([nexp, ncomp]) act along the exposure axis
of every pixel column.  A column is live when b > 0 at every exposure, otherwise dead and all NaN; for a live column

    c_j = sum_v fwd[s][j][v] g[v][p]      r_v = sum_j back[s][v][j] c_j      g'[v][p] = g[v][p] - r_v

and the filtered moments are the seven sums with g' in place of g over the pixels with a value and w > 0.

    Filter(fwd, back)                                    a filter; to_c() its trx_filter
    svd_filter(data, seg_first, ncomp)                   back = U, fwd = U^T: each segment's leading left singular vectors
    filter_reference(pairs, obs, filt)                   g' by the definition, in np.longdouble and rounded; dead columns NaN
    filter_abs_reference(pairs, obs, filt)               |g| + |back| (|fwd| |g|): the scale of a value's rounding error
    reference_values(values, obs)                        the moments from a value matrix [nexp, npix], sums by math.fsum
    abs_reference_values(values, obs)                    the same with |f| and |values|

The weighted filter (Engine.set_weighted_filter; trx_set_weighted_filter), the filter slot's second kind: every pixel column
is projected by least squares under its OWN weights w[v] = weight[v][p], with its segment's time vectors U = basis[s]
([nexp, ncomp]): g' = g - U (U^T diag(w) U)^-1 U^T diag(w) g.  The column's normal matrix is factorised (L D L^T) when the
filter is installed; a pivot at or below 2^-26 of its diagonal entry is singular and the column dead (NaN), as is a column
with b <= 0 at any exposure.  The operations and their order are stated in include/transit_hip.h.

    WeightedFilter(basis)                                a weighted filter; to_c() its trx_wfilter
    svd_basis(data, seg_first, ncomp)                    the back of svd_filter: each segment's leading left singular vectors
    sysrem_basis(data, weight, seg_first, ncomp, niter)  SYSREM's time vectors (Tamuz et al. 2005), normalised
    weighted_factor(obs, wf)                             (L, D, live) of every column: the install step, bit for bit the device's
    weighted_pivots(obs, wf)                             every pivot's share D_j / N_jj of its diagonal entry
    weighted_filter_reference(pairs, obs, wf)            g' [nexp, npix] in double in the definition's order: bit for bit the device's
    weighted_filter_exact(pairs, obs, wf)                the same projection in np.longdouble, rounded at the end
    weighted_filter_bound(pairs, obs, wf)                how far a double evaluation can lie from the exact projection

Detrending the observed exposures themselves on the device (Engine.detrend_observed; trx_detrend_observed): a model is
multiplied into the RAW data (optional), SYSREM runs on them per segment, the residuals become the observed data and the
weighted filter of the fitted basis the filter.  The operations and their order are stated in include/transit_hip.h; the
mirrors here follow them bit for bit, the row sums included (64 lane sums, then the wave's butterfly).

    wave_sum(lanes)                                      the butterfly over 64 lane sums [..., 64]: partner lane ^ 32, 16, 8, 4, 2, 1
    row_sum(terms)                                       the sum of terms [..., n] in the device's order: lanes, then wave_sum
    inject_reference(pairs, obs, p0, p1)                 f0 = F * (p0 g + p1) where b > 0, F elsewhere
    sysrem_reference(data, weight, seg_first, ncomp, niter)      (basis, coef, resid): the mirror of the device's SYSREM

The same call with a principal-component analysis in time in SYSREM's place (Engine.pca_observed; trx_pca_observed): the
Gram matrix of each segment's whole columns, its eigenvectors by a fixed number of Jacobi sweeps in a fixed parallel order.

    jacobi_rounds(nexp)                                  the rounds of one sweep: lists of disjoint pairs (p, q), p < q < nexp
    pca_reference(data, weight, seg_first, ncomp, nsweep)        (basis, coef, resid, eigen, offdiag, nwhole): the mirror

The same call with a regression on GIVEN time vectors in SYSREM's place (Engine.regress_observed; trx_regress_observed):
every pixel column fitted by weighted least squares with its segment's vectors -- the weighted filter's projector applied
to the data --, then optionally a few SYSREM components on the residuals.

    regress_reference(f0, weight, seg_first, vectors)    (coef, resid, nsingular): the mirror; a singular column keeps f0
    time_basis(x, degree)                                [nexp, degree + 1]: the powers of the centred, scaled x (the airmass)

Normalising the observed set ahead of either (Engine.set_normalise / Engine.normalise_observed; trx_set_normalise /
trx_normalise_observed): step 1b of the detrending calls, between the injection and the fit.  Every (exposure, segment) row
is divided by a quantile of its live data, every column by (or less) its mean in time, single entries are clipped.

    Normalise(row_kind, col_kind, quantile=0.5, clip=0.0)        a recipe; to_c() its trx_normalise
    normalise_reference(f0, weight, seg_first, nm)               (data, rowscale, centre, nclipped, nbad): the mirror, the
                                                                 quantile from a full sort of the live values

The detection map with the filter applied to every cell's own model matrix (Engine.run_filtered_map /
Batch.run_filtered_map; trx_run_filtered_map): a cell takes at every exposure the row of the lag NEAREST to its velocity,
that matrix goes through the filter and the moments above, and the cell is the statistic added over the segments and
then over the exposures, both in order.

    nearest_lags(vm)                                     [nkp, nvsys, nexp]: the lag every cell takes at every exposure, -1 outside
    cell_value(mom, vm)                                  a cell from its moments [nexp, nseg, 7]
    cell_bound(mom, vm)                                  how far two double evaluations of cell_value can lie apart
    filtered_map_reference(pairs, obs, filt, vm)         the whole definition in numpy from run_pixels(lags)' pairs

The same map under the exposure table (Engine.run_exposed_map / Batch.run_exposed_map; trx_run_exposed_map): a pixel row
is a pair (lag, exposure), so that the table's scale and smear act on the model before the filter.

    exposed_map_rows(vm)                                 (lo, hi, base, R): the span of lags per exposure, the rows' bases, their number
    exposed_map_reference(pairs_lv, obs, filt, vm, hp)   the whole definition in numpy from run_exposed's pairs per lag

The high-pass along the pixel axis (Engine.set_highpass / Engine.run_highpassed; trx_set_highpass / trx_run_highpassed):
a symmetric tap table taps[0 .. half] (finite, >= 0, taps[0] > 0) over the observed set's segments.  For a row of pairs
and a live pixel p (b > 0) of a segment, over the live pixels p + k of that segment, k = -half .. half in that order,

    g'_p = g_p - (sum taps[|k|] g_{p+k}) / (sum taps[|k|])

every operation rounded once; a dead pixel is NaN.  With it installed run_moments, run_filtered_moments, run_trail and
run_velocity_map take g' where they took g.

    HighPass(taps)                                       a high-pass; to_c() its trx_highpass
    gaussian_highpass(sigma_pix, cut=3.0)                taps exp(-k^2 / (2 sigma^2)), half = floor(cut * sigma)
    boxcar_highpass(width)                               width equal taps (width odd)
    highpass_reference(pairs, obs, hp)                   g' [n, npix] by the definition, bit for bit the device's; dead NaN
    highpass_pairs(values)                               the pairs (g', 1) / (0, 0) of such values: what reference,
                                                         trail_reference and filter_reference take with a gain-free set
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _abi, pixels as _pixels

NMOMENT = _abi.NMOMENT
N, W, WG, WGG, WF, WFG, WFF = range(NMOMENT)


def segments(lengths) -> np.ndarray:
    """seg_first ([nseg + 1], int64) of segments of the given lengths, laid end to end from pixel 0."""
    n = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if np.any(n < 0):
        raise ValueError("segments: a negative length")
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


@dataclass
class Observed:
    """One trx_observed: segment bounds [nseg + 1], data [nexp, npix] (finite), weights [nexp, npix] (finite, >= 0;
    None: all 1) and gain [npix] (finite; None: 1)."""
    seg_first: np.ndarray
    data: np.ndarray
    weight: Optional[np.ndarray] = None
    gain: Optional[np.ndarray] = None

    def __post_init__(self):
        self.seg_first = np.ascontiguousarray(self.seg_first, dtype=np.int64).reshape(-1)
        self.data = np.ascontiguousarray(self.data, dtype=np.float64)
        if self.data.ndim != 2:
            raise ValueError("Observed: data of shape [nexp][npix]")
        if self.weight is not None:
            self.weight = np.ascontiguousarray(self.weight, dtype=np.float64)
            if self.weight.shape != self.data.shape:
                raise ValueError("Observed: weight of the shape of data")
        if self.gain is not None:
            self.gain = np.ascontiguousarray(self.gain, dtype=np.float64).reshape(-1)
            if self.gain.size != self.data.shape[1]:
                raise ValueError("Observed: one gain per pixel")
        if self.seg_first.size < 1:
            raise ValueError("Observed: seg_first of nseg + 1 entries")

    @property
    def nexp(self) -> int:
        return int(self.data.shape[0])

    @property
    def npix(self) -> int:
        return int(self.data.shape[1])

    @property
    def nseg(self) -> int:
        return int(self.seg_first.size) - 1

    def to_c(self):
        """The trx_observed of the set (the arrays stay owned by this object)."""
        c = _abi.TrxObserved()
        c.nexp, c.nseg = self.nexp, self.nseg
        c.seg_first = self.seg_first.ctypes.data_as(_abi.c_int64_p)
        c.data = self.data.ctypes.data_as(_abi.c_double_p)
        c.weight = self.weight.ctypes.data_as(_abi.c_double_p) if self.weight is not None else None
        c.gain = self.gain.ctypes.data_as(_abi.c_double_p) if self.gain is not None else None
        return c


def _model(pairs, obs: Observed):
    """(g, b > 0): the model values gain_p * (a / b) -- one division, one product, each rounded once -- where b > 0
    (0 elsewhere), and where that is"""
    pairs = np.asarray(pairs, dtype=np.float64)
    if pairs.shape != (obs.nexp, obs.npix, 2):
        raise ValueError("pairs of shape [nexp][npix][2]")
    a, b = pairs[..., 0], pairs[..., 1]
    gain = obs.gain if obs.gain is not None else np.ones(obs.npix)
    on = b > 0
    return np.where(on, gain[None, :] * (a / np.where(on, b, 1.0)), 0.0), on


def _moments(pairs, obs: Observed, absolute: bool) -> np.ndarray:
    g, on = _model(pairs, obs)
    return _sums(g, on, obs, absolute)


def _sums(g, has, obs: Observed, absolute: bool) -> np.ndarray:
    """the seven sums per (v, s) of the model values g over the pixels that have one (has) and w > 0"""
    w = obs.weight if obs.weight is not None else np.ones_like(obs.data)
    use = has & (w > 0)
    f = obs.data
    if absolute:
        g, f = np.abs(g), np.abs(f)
    wg, wf = w * g, w * f
    terms = (np.ones_like(w), w, wg, wg * g, wf, wf * g, wf * f)
    out = np.zeros((obs.nexp, obs.nseg, NMOMENT))
    for v in range(obs.nexp):
        for s in range(obs.nseg):
            k = np.arange(obs.seg_first[s], obs.seg_first[s + 1])
            k = k[use[v, k]]
            for c, t in enumerate(terms):
                out[v, s, c] = math.fsum(t[v, k])
    return out


def reference(pairs, obs: Observed) -> np.ndarray:
    """The definition: [nexp, nseg, 7] from the pixel pairs [nexp, npix, 2] of a run and the observed set -- the
    terms in numpy (every operation rounded once, as on the device), the sums by math.fsum."""
    return _moments(pairs, obs, False)


def abs_reference(pairs, obs: Observed) -> np.ndarray:
    """reference with |f| and |g|: the sums of the absolute terms, which the rounding error of a sum is relative to."""
    return _moments(pairs, obs, True)


def chi2(mom, a: float = 1.0, b: float = 0.0) -> np.ndarray:
    """sum of w (f - a g - b)^2 over the contributing pixels, per (v, s):
    m6 - 2a m5 - 2b m4 + a^2 m3 + 2ab m2 + b^2 m1."""
    m = np.asarray(mom, dtype=np.float64)
    return m[..., WFF] - 2 * a * m[..., WFG] - 2 * b * m[..., WF] + a * a * m[..., WGG] + 2 * a * b * m[..., WG] + b * b * m[..., W]


def central(mom):
    """(n, s_f^2, s_g^2, R, ok) per (v, s): the weighted mean-subtracted variances of f and g and their covariance,
    sum w (x - <x>)(y - <y>) / sum w with <x> = sum w x / sum w; ok is False for a row with n < 2 or a variance that
    is not positive (there the three are nan)."""
    m = np.asarray(mom, dtype=np.float64)
    n, sw = m[..., N], m[..., W]
    with np.errstate(divide="ignore", invalid="ignore"):
        mf, mg = m[..., WF] / sw, m[..., WG] / sw
        sf2 = m[..., WFF] / sw - mf * mf
        sg2 = m[..., WGG] / sw - mg * mg
        r = m[..., WFG] / sw - mf * mg
        ok = (n >= 2) & (sf2 > 0) & (sg2 > 0)
    nan = np.full(m.shape[:-1], np.nan)
    return n, np.where(ok, sf2, nan), np.where(ok, sg2, nan), np.where(ok, r, nan), ok


def ccf(mom) -> np.ndarray:
    """The weighted Pearson correlation coefficient of f and g per (v, s), R / sqrt(s_f^2 s_g^2); nan for a row with
    fewer than two contributing pixels or a zero variance."""
    _, sf2, sg2, r, ok = central(mom)
    with np.errstate(invalid="ignore"):
        return r / np.sqrt(sf2 * sg2)


def loglike_bl19(mom, scale: float = 1.0) -> np.ndarray:
    """The log-likelihood of Brogi & Line (2019) per (v, s): -n/2 log(s_f^2 - 2 scale R + scale^2 s_g^2); nan for a
    row with fewer than two contributing pixels, a zero variance or an argument of the logarithm that is not
    positive."""
    n, sf2, sg2, r, ok = central(mom)
    with np.errstate(invalid="ignore", divide="ignore"):
        arg = sf2 - 2 * scale * r + scale * scale * sg2
        return np.where(arg > 0, -0.5 * n * np.log(np.where(arg > 0, arg, 1.0)), np.nan)


def chi2_sum(mom, a: float = 1.0, b: float = 0.0) -> float:
    """chi2 added over every (v, s)."""
    return float(np.sum(chi2(mom, a, b)))


def ccf_sum(mom) -> float:
    """ccf added over the (v, s) rows that have one: rows for which ccf is nan (fewer than two contributing pixels,
    a zero variance) are SKIPPED, not counted as zero."""
    return float(np.nansum(ccf(mom)))


def loglike_bl19_sum(mom, scale: float = 1.0) -> float:
    """loglike_bl19 added over the (v, s) rows that have one: rows for which it is nan (fewer than two contributing
    pixels, a zero variance) are SKIPPED."""
    return float(np.nansum(loglike_bl19(mom, scale)))


def _trail(pairs, obs: Observed, absolute: bool) -> np.ndarray:
    pairs = np.asarray(pairs, dtype=np.float64)
    if pairs.ndim != 3 or pairs.shape[1:] != (obs.npix, 2):
        raise ValueError("pairs of shape [nlag][npix][2]")
    out = np.zeros((pairs.shape[0], obs.nexp, obs.nseg, NMOMENT))
    for l in range(pairs.shape[0]):
        out[l] = _moments(np.broadcast_to(pairs[l], (obs.nexp, obs.npix, 2)), obs, absolute)
    return out


def trail_reference(pairs, obs: Observed) -> np.ndarray:
    """The definition of the trail: [nlag, nexp, nseg, 7] from the pixel pairs [nlag, npix, 2] of a run at the lags
    and the observed set -- lag l is reference() with that lag's pairs at every exposure."""
    return _trail(pairs, obs, False)


def trail_abs_reference(pairs, obs: Observed) -> np.ndarray:
    """trail_reference with |f| and |g| (abs_reference per lag)."""
    return _trail(pairs, obs, True)


def lag_grid(v_lo: float, v_hi: float, step: float):
    """(lag_kms, lags): the velocities v_lo, v_lo + step, ... up to v_hi (km/s; v_hi included when a whole number of
    steps away, to rounding) and the Doppler factor pixels.shift of each -- what run_trail takes."""
    if not (step > 0) or not (v_hi >= v_lo):
        raise ValueError("lag_grid: step > 0 and v_hi >= v_lo")
    n = int(math.floor((v_hi - v_lo) / step * (1.0 + 1e-12) + 1e-9)) + 1
    kms = v_lo + step * np.arange(n, dtype=np.float64)
    return kms, np.array([_pixels.shift(v) for v in kms])


def velocity_map(trail, lag_kms, v_planet, stat=ccf) -> np.ndarray:
    """The detection map of a trail [nlag, nexp, nseg, 7] over lags at the velocities lag_kms ([nlag], increasing):
    v_planet ([..., nexp]) is the planet's velocity at every exposure for every map cell, e.g.
    vsys[None, :, None] + kp[:, None, None] * sin(2 pi phase).  stat (ccf, loglike_bl19, chi2, ...) is applied to the
    trail and added over the segments -- rows it leaves undefined (nan) are SKIPPED, as the *_sum helpers skip them
    -- which gives [nlag, nexp]; that is interpolated linearly in lag velocity at each exposure's velocity and added
    over the exposures.  A cell with any velocity outside [lag_kms[0], lag_kms[-1]] is nan."""
    trail = np.asarray(trail, dtype=np.float64)
    kms = np.asarray(lag_kms, dtype=np.float64).reshape(-1)
    vp = np.asarray(v_planet, dtype=np.float64)
    if trail.ndim != 4 or trail.shape[0] != kms.size or trail.shape[3] != NMOMENT:
        raise ValueError("velocity_map: trail of shape [nlag][nexp][nseg][7], one lag velocity per lag")
    if kms.size > 1 and not np.all(np.diff(kms) > 0):
        raise ValueError("velocity_map: lag_kms must increase")
    if vp.ndim < 1 or vp.shape[-1] != trail.shape[1]:
        raise ValueError("velocity_map: v_planet of shape [..., nexp]")
    per = np.nansum(np.asarray(stat(trail), dtype=np.float64), axis=2)      # [nlag, nexp]
    inside = (vp >= kms[0]) & (vp <= kms[-1])
    out = np.zeros(vp.shape[:-1])
    for v in range(trail.shape[1]):
        x = np.where(inside[..., v], vp[..., v], kms[0])
        if kms.size == 1:
            out += per[0, v]
            continue
        k = np.clip(np.searchsorted(kms, x, side="right") - 1, 0, kms.size - 2)
        t = (x - kms[k]) / (kms[k + 1] - kms[k])
        out += per[k, v] + t * (per[k + 1, v] - per[k, v])
    return np.where(np.all(inside, axis=-1), out, np.nan)


STATS = {"ccf": _abi.STAT_CCF, "loglike_bl19": _abi.STAT_LOGLIKE_BL19, "chi2": _abi.STAT_CHI2}


@dataclass
class VelocityMap:
    """One trx_vmap: the lag grid lag_kms ([nlag] km/s, strictly increasing; lag, their Doppler factors pixels.shift,
    is filled in), the map's axes kp ([nkp]) and vsys ([nvsys]) in km/s, orbit ([nexp]: what multiplies Kp at every
    exposure, sin(2 pi phase) for a circular orbit), offset ([nexp] km/s added at every exposure, or None) and the
    statistic: "ccf", "loglike_bl19" (scale) or "chi2" (a, b)."""
    lag_kms: np.ndarray
    kp: np.ndarray
    vsys: np.ndarray
    orbit: np.ndarray
    offset: Optional[np.ndarray] = None
    stat: str = "ccf"
    scale: float = 1.0
    a: float = 1.0
    b: float = 0.0
    lag: Optional[np.ndarray] = None

    def __post_init__(self):
        flat = lambda x: np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        self.lag_kms, self.kp, self.vsys, self.orbit = flat(self.lag_kms), flat(self.kp), flat(self.vsys), flat(self.orbit)
        if self.offset is not None:
            self.offset = flat(self.offset)
            if self.offset.size != self.orbit.size:
                raise ValueError("VelocityMap: one offset per exposure")
        if self.stat not in STATS:
            raise ValueError("VelocityMap: stat is one of %s" % ", ".join(sorted(STATS)))
        self.lag = np.array([_pixels.shift(v) for v in self.lag_kms]) if self.lag is None else flat(self.lag)
        if self.lag.size != self.lag_kms.size:
            raise ValueError("VelocityMap: one lag per lag velocity")

    @property
    def nlag(self) -> int:
        return int(self.lag_kms.size)

    @property
    def nkp(self) -> int:
        return int(self.kp.size)

    @property
    def nvsys(self) -> int:
        return int(self.vsys.size)

    @property
    def nexp(self) -> int:
        return int(self.orbit.size)

    @property
    def params(self):
        """(p0, p1) of the trx_vmap: (scale, 0) for loglike_bl19, (a, b) for chi2, (0, 0) for ccf"""
        return {"ccf": (0.0, 0.0), "loglike_bl19": (float(self.scale), 0.0), "chi2": (float(self.a), float(self.b))}[self.stat]

    def statistic(self, mom) -> np.ndarray:
        """the statistic of moments [..., 7]: ccf, loglike_bl19 or chi2 with this map's parameters"""
        return {"ccf": lambda m: ccf(m), "loglike_bl19": lambda m: loglike_bl19(m, float(self.scale)),
                "chi2": lambda m: chi2(m, float(self.a), float(self.b))}[self.stat](mom)

    def to_c(self):
        """The trx_vmap of the map (the arrays stay owned by this object)."""
        c = _abi.TrxVmap()
        c.stat, c.nlag = STATS[self.stat], self.nlag
        c.p0, c.p1 = self.params
        c.lag = self.lag.ctypes.data_as(_abi.c_double_p)
        c.lag_kms = self.lag_kms.ctypes.data_as(_abi.c_double_p)
        c.nkp, c.nvsys = self.nkp, self.nvsys
        c.kp = self.kp.ctypes.data_as(_abi.c_double_p)
        c.vsys = self.vsys.ctypes.data_as(_abi.c_double_p)
        c.orbit = self.orbit.ctypes.data_as(_abi.c_double_p)
        c.offset = self.offset.ctypes.data_as(_abi.c_double_p) if self.offset is not None else None
        return c


def _check_trail(trail, vm: VelocityMap) -> np.ndarray:
    trail = np.asarray(trail, dtype=np.float64)
    if trail.ndim != 4 or trail.shape[0] != vm.nlag or trail.shape[1] != vm.nexp or trail.shape[3] != NMOMENT:
        raise ValueError("trail of shape [nlag][nexp][nseg][7] with the map's nlag and nexp")
    return trail


def trail_statistic(trail, vm: VelocityMap) -> np.ndarray:
    """per [nlag, nexp] by the definition of trx_run_velocity_map: the map's statistic of every trail row, added over
    the segments s = 0, 1, ... IN THAT ORDER, one addition each, from +0; rows the statistic leaves undefined (nan) are
    skipped.  (velocity_map adds them with np.nansum, whose order is pairwise: the same sum to rounding.)"""
    st = np.asarray(vm.statistic(_check_trail(trail, vm)), dtype=np.float64)
    per = np.zeros(st.shape[:2])
    for s in range(st.shape[2]):
        with np.errstate(invalid="ignore"):
            per = np.where(np.isnan(st[:, :, s]), per, per + st[:, :, s])
    return per


def _tracks(vm: VelocityMap) -> np.ndarray:
    """x [nkp, nvsys, nexp]: (kp * orbit + vsys) + offset, the last addition only with an offset"""
    x = vm.kp[:, None, None] * vm.orbit[None, None, :] + vm.vsys[None, :, None]
    return x + vm.offset[None, None, :] if vm.offset is not None else x


def _locate(kms, x):
    """(inside, k, t) of the velocities x on the grid kms: trx_run_velocity_map's step 3 (outside: k = 0, t = 0)"""
    with np.errstate(invalid="ignore"):
        inside = (x >= kms[0]) & (x <= kms[-1])
    if kms.size < 2:
        return inside, np.zeros(x.shape, dtype=np.int64), np.zeros(x.shape)
    xi = np.where(inside, x, kms[0])
    k = np.clip(np.searchsorted(kms, xi, side="right") - 1, 0, kms.size - 2)
    t = (xi - kms[k]) / (kms[k + 1] - kms[k])
    return inside, k, np.where(inside, t, 0.0)


def map_from_per(per, vm: VelocityMap) -> np.ndarray:
    """The map [nkp, nvsys] from per [nlag, nexp] by the definition of trx_run_velocity_map: exposure after exposure,
    per[k, v] + t * (per[k + 1, v] - per[k, v]) at the cell's velocity, added in that order from +0; a cell with a
    velocity outside the lag grid, or not finite, is nan.  Engine.run_velocity_map's map is this of its per, bit for
    bit."""
    per = np.asarray(per, dtype=np.float64)
    if per.shape != (vm.nlag, vm.nexp):
        raise ValueError("per of shape [nlag][nexp]")
    inside, k, t = _locate(vm.lag_kms, _tracks(vm))
    out = np.zeros((vm.nkp, vm.nvsys))
    for v in range(vm.nexp):
        if vm.nlag < 2:
            out = out + per[0, v]
            continue
        kv, tv = k[..., v], t[..., v]
        with np.errstate(invalid="ignore"):
            out = out + (per[kv, v] + tv * (per[kv + 1, v] - per[kv, v]))
    return np.where(np.all(inside, axis=-1), out, np.nan)


def map_reference(trail, vm: VelocityMap) -> np.ndarray:
    """The map of a trail by the definition, all in numpy: map_from_per(trail_statistic(trail, vm), vm)."""
    return map_from_per(trail_statistic(trail, vm), vm)


_EPS = 2.0 ** -52


def _abs_rows(trail, vm: VelocityMap) -> np.ndarray:
    """A [nlag, nexp]: the sum over the segments of |statistic| (undefined rows: nothing)"""
    return np.nansum(np.abs(np.asarray(vm.statistic(_check_trail(trail, vm)), dtype=np.float64)), axis=2)


def per_bound(trail, vm: VelocityMap) -> np.ndarray:
    """[nlag, nexp]: how far per of the device may lie from trail_statistic of the same trail -- the row part of
    map_bound.  Both add the same nseg terms in the same order, so only the terms can differ.  A ccf or chi2 term uses
    +, -, *, / and sqrt alone, all correctly rounded on either side: the same bits, and 4 * 2^-52 * A, A the sum of the
    |terms| of the row, is a safety net.  A loglike_bl19 term is (-n/2) log(arg) with the same arg on both sides; the
    device's log is within 3 ulp and numpy's within 1, the product rounds once on each side: 5 * 2^-52 |term| at the
    most; nseg additions of terms that differ give partial sums that differ, each rounded: nseg * 2^-52 * A more."""
    a = _abs_rows(trail, vm)
    nseg = np.asarray(trail).shape[2]
    return (5 + nseg if vm.stat == "loglike_bl19" else 4) * _EPS * a


def map_bound(trail, vm: VelocityMap) -> np.ndarray:
    """[nkp, nvsys] (nan where the cell is): how far two double evaluations of a map cell from one trail can lie apart
    when each adds the segments in ANY order (trail_statistic in index order, velocity_map pairwise, the device in
    index order) and the exposures in index order.  With A[l, v] the sum of the |statistics| of the rows (l, v, .) and
    S = sum over v of A[k_v, v] + A[k_v + 1, v] -- the absolute terms that enter the cell:

      - per: each side's statistic of a row is within c * 2^-53 |term| of the exact one (c = 4: ccf and chi2 are at most
        a dozen correctly rounded operations but agree bit for bit in practice; c = 5 for loglike_bl19, see per_bound),
        and a sum of nseg terms in any order is within (nseg - 1) 2^-53 A of the exact sum of its terms: two sides lie
        at most (c + nseg) 2^-52 A apart.  The interpolation passes a difference of the two rows on with weights
        1 - t and t in [0, 1]: at most (c + nseg) 2^-52 (A[k] + A[k+1]) per exposure;
      - the term per[k] + t (per[k+1] - per[k]): t from two operations, then a difference, a product and a sum, each
        within 2^-53 of a magnitude of at most |per[k]| + |per[k+1]| <= A[k] + A[k+1]: 5 * 2^-53 per side;
      - the sum of nexp terms in order: (nexp - 1) 2^-53 of the sum of the |terms| per side, each |term| at most
        max(|per[k]|, |per[k+1]|).

    Together (c + nseg + 5 + nexp) 2^-52 S, to first order in 2^-52 -- below the (nseg + nexp + 16) 2^-52 S that the
    interface promises at the most."""
    trail = _check_trail(trail, vm)
    a = _abs_rows(trail, vm)
    nseg = trail.shape[2]
    inside, k, _ = _locate(vm.lag_kms, _tracks(vm))
    s = np.zeros((vm.nkp, vm.nvsys))
    for v in range(vm.nexp):
        s += a[0, v] if vm.nlag < 2 else a[k[..., v], v] + a[k[..., v] + 1, v]
    c = 5 if vm.stat == "loglike_bl19" else 4
    return np.where(np.all(inside, axis=-1), (c + nseg + 5 + vm.nexp) * _EPS * s, np.nan)


@dataclass
class Filter:
    """One trx_filter: the coefficients fwd [nseg, ncomp, nexp] and the basis back [nseg, nexp, ncomp] (finite; a
    segment that wants fewer components pads with zeros)."""
    fwd: np.ndarray
    back: np.ndarray

    def __post_init__(self):
        self.fwd = np.ascontiguousarray(self.fwd, dtype=np.float64)
        self.back = np.ascontiguousarray(self.back, dtype=np.float64)
        if self.fwd.ndim != 3 or self.back.ndim != 3:
            raise ValueError("Filter: fwd of shape [nseg][ncomp][nexp], back of shape [nseg][nexp][ncomp]")
        if self.back.shape != (self.fwd.shape[0], self.fwd.shape[2], self.fwd.shape[1]):
            raise ValueError("Filter: back of the shape of fwd with its last two axes exchanged")

    @property
    def nseg(self) -> int:
        return int(self.fwd.shape[0])

    @property
    def ncomp(self) -> int:
        return int(self.fwd.shape[1])

    @property
    def nexp(self) -> int:
        return int(self.fwd.shape[2])

    def to_c(self):
        """The trx_filter of the filter (the arrays stay owned by this object)."""
        c = _abi.TrxFilter()
        c.ncomp, c.pad = self.ncomp, 0
        c.fwd = self.fwd.ctypes.data_as(_abi.c_double_p)
        c.back = self.back.ctypes.data_as(_abi.c_double_p)
        return c


def svd_filter(data, seg_first, ncomp: int) -> Filter:
    """The filter that takes the leading ncomp principal components in time out of every segment: per segment the
    leading left singular vectors U ([nexp, ncomp]) of data[:, segment], back = U and fwd = U^T.  A segment with fewer
    singular vectors than ncomp (an empty one: none) pads with zeros."""
    data = np.asarray(data, dtype=np.float64)
    seg = np.asarray(seg_first, dtype=np.int64).reshape(-1)
    nexp, nseg = data.shape[0], seg.size - 1
    back = np.zeros((nseg, nexp, ncomp))
    for s in range(nseg):
        if seg[s + 1] > seg[s]:
            u = np.linalg.svd(data[:, seg[s]:seg[s + 1]], full_matrices=False)[0][:, :ncomp]
            back[s, :, :u.shape[1]] = u
    return Filter(np.ascontiguousarray(back.transpose(0, 2, 1)), back)


def _check_filter(obs: Observed, filt: Filter):
    if (filt.nseg, filt.nexp) != (obs.nseg, obs.nexp):
        raise ValueError("filter of the observed set's nseg and nexp")


def filter_reference(pairs, obs: Observed, filt: Filter) -> np.ndarray:
    """The definition: g' [nexp, npix] from the pixel pairs [nexp, npix, 2] of a run -- g in numpy as the moments take
    it, the projection in np.longdouble, rounded to double at the end; a column with b <= 0 at any exposure is NaN."""
    _check_filter(obs, filt)
    g, on = _model(pairs, obs)
    live = np.all(on, axis=0)
    out = np.full(g.shape, np.nan)
    gl = g.astype(np.longdouble)
    for s in range(obs.nseg):
        k = np.arange(obs.seg_first[s], obs.seg_first[s + 1])
        k = k[live[k]]
        c = filt.fwd[s].astype(np.longdouble) @ gl[:, k]
        out[:, k] = (gl[:, k] - filt.back[s].astype(np.longdouble) @ c).astype(np.float64)
    return out


def filter_abs_reference(pairs, obs: Observed, filt: Filter) -> np.ndarray:
    """|g| + |back| (|fwd| |g|) [nexp, npix]: what the rounding error of a filtered value is relative to (NaN in the
    dead columns)."""
    _check_filter(obs, filt)
    g, on = _model(pairs, obs)
    live = np.all(on, axis=0)
    out = np.full(g.shape, np.nan)
    for s in range(obs.nseg):
        k = np.arange(obs.seg_first[s], obs.seg_first[s + 1])
        k = k[live[k]]
        out[:, k] = np.abs(g[:, k]) + np.abs(filt.back[s]) @ (np.abs(filt.fwd[s]) @ np.abs(g[:, k]))
    return out


def _values(values, obs: Observed):
    values = np.asarray(values, dtype=np.float64)
    if values.shape != (obs.nexp, obs.npix):
        raise ValueError("values of shape [nexp][npix]")
    has = ~np.isnan(values)
    return np.where(has, values, 0.0), has


def reference_values(values, obs: Observed) -> np.ndarray:
    """The moments [nexp, nseg, 7] of a matrix of model values [nexp, npix] (gain and division in them already, NaN:
    no value) against the observed set: the terms and the sums of reference()."""
    return _sums(*_values(values, obs), obs, False)


def abs_reference_values(values, obs: Observed) -> np.ndarray:
    """reference_values with |f| and |values|."""
    return _sums(*_values(values, obs), obs, True)


def nearest_lags(vm: VelocityMap) -> np.ndarray:
    """[nkp, nvsys, nexp] int: the lag NEAREST to every cell's velocity at every exposure, as trx_run_filtered_map takes
    it -- _locate's k, or k + 1 when t > 0.5 (a tie goes to the lower lag; one lag: 0) -- and -1 where the velocity is
    outside the lag grid or not finite.  Built on _tracks and _locate, whose operations are the device's: the same
    index on either side, ties included."""
    inside, k, t = _locate(vm.lag_kms, _tracks(vm))
    return np.where(inside, k + (t > 0.5), -1).astype(np.int64)


def cell_value(mom, vm: VelocityMap) -> float:
    """Point 5 of trx_run_filtered_map on a cell's moments [nexp, nseg, 7]: per exposure the map's statistic of the rows
    added over the segments s = 0, 1, ... IN THAT ORDER from +0, undefined rows (nan) skipped; then those sums added over
    the exposures in order from +0."""
    mom = np.asarray(mom, dtype=np.float64)
    if mom.ndim != 3 or mom.shape[0] != vm.nexp or mom.shape[2] != NMOMENT:
        raise ValueError("mom of shape [nexp][nseg][7] with the map's nexp")
    st = np.asarray(vm.statistic(mom), dtype=np.float64)
    per = np.zeros(mom.shape[0])
    for s in range(mom.shape[1]):
        with np.errstate(invalid="ignore"):
            per = np.where(np.isnan(st[:, s]), per, per + st[:, s])
    out = 0.0
    for v in range(mom.shape[0]):
        out = out + float(per[v])
    return out


def cell_bound(mom, vm: VelocityMap) -> float:
    """How far two double evaluations of point 5 (cell_value on the host, k_cell_stat on the device) of the SAME moments
    [nexp, nseg, 7] can lie apart: map_bound's t = 0, single-row case.  With A_v the sum over the segments of
    |statistic| of the rows (v, .) and S the sum of the A_v:

      - each side's statistic of a row is within c * 2^-53 |term| of the exact one (c = 4 for ccf and chi2, a dozen
        correctly rounded operations that agree bit for bit in practice; c = 5 for loglike_bl19, see per_bound), and a
        sum of nseg terms is within (nseg - 1) 2^-53 A_v of the exact sum of its terms: two sides lie at most
        (c + nseg) 2^-52 A_v apart in per_v;
      - there is no interpolation: the cell takes one row per exposure, and per_v enters the sum as it stands;
      - the sum of nexp terms in order: (nexp - 1) 2^-53 of the sum of the |per_v| <= S per side.

    Together (c + nseg + nexp) 2^-52 S, to first order in 2^-52."""
    mom = np.asarray(mom, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        s = float(np.nansum(np.abs(np.asarray(vm.statistic(mom), dtype=np.float64))))
    c = 5 if vm.stat == "loglike_bl19" else 4
    return (c + mom.shape[1] + mom.shape[0]) * _EPS * s


@dataclass
class WeightedFilter:
    """One trx_wfilter: the time vectors basis [nseg, nexp, ncomp] (finite) of every segment.  The weights of the
    projection are the observed set's."""
    basis: np.ndarray

    def __post_init__(self):
        self.basis = np.ascontiguousarray(self.basis, dtype=np.float64)
        if self.basis.ndim != 3:
            raise ValueError("WeightedFilter: basis of shape [nseg][nexp][ncomp]")

    @property
    def nseg(self) -> int:
        return int(self.basis.shape[0])

    @property
    def nexp(self) -> int:
        return int(self.basis.shape[1])

    @property
    def ncomp(self) -> int:
        return int(self.basis.shape[2])

    def to_c(self):
        """The trx_wfilter of the filter (the array stays owned by this object)."""
        c = _abi.TrxWfilter()
        c.ncomp, c.pad = self.ncomp, 0
        c.basis = self.basis.ctypes.data_as(_abi.c_double_p)
        return c


def svd_basis(data, seg_first, ncomp: int) -> np.ndarray:
    """[nseg, nexp, ncomp]: each segment's leading left singular vectors, the `back` of svd_filter.  A segment with fewer
    singular vectors than ncomp keeps zero vectors there -- singular pivots under a weighted filter."""
    return svd_filter(data, seg_first, ncomp).back


def sysrem_basis(data, weight, seg_first, ncomp: int, niter: int = 10) -> np.ndarray:
    """[nseg, nexp, ncomp]: the time vectors of SYSREM (Tamuz, Mazeh & Zucker 2005) per segment, one component after
    another.  With r the segment's residuals [nexp, n] (the data at first) and w their weights (None: all 1), a
    component starts from a = 1 and alternates, niter times,

        c_p = sum_v w r a / sum_v w a^2        a_v = sum_p w r c / sum_p w c^2        (0 where the denominator is 0)

    then a is normalised to unit length (c takes the factor), kept as the component, and a c^T leaves the residuals."""
    data = np.asarray(data, dtype=np.float64)
    w_all = np.ones_like(data) if weight is None else np.asarray(weight, dtype=np.float64)
    seg = np.asarray(seg_first, dtype=np.int64).reshape(-1)
    nexp, nseg = data.shape[0], seg.size - 1
    out = np.zeros((nseg, nexp, ncomp))

    def ratio(num, den):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)

    for s in range(nseg):
        r, w = data[:, seg[s]:seg[s + 1]].copy(), w_all[:, seg[s]:seg[s + 1]]
        if r.shape[1] == 0:
            continue
        for i in range(ncomp):
            a = np.ones(nexp)
            c = np.zeros(r.shape[1])
            for _ in range(niter):
                c = ratio(np.sum(w * r * a[:, None], axis=0), np.sum(w * (a * a)[:, None], axis=0))
                a = ratio(np.sum(w * r * c[None, :], axis=1), np.sum(w * (c * c)[None, :], axis=1))
            norm = float(np.sqrt(np.sum(a * a)))
            if norm > 0:
                a, c = a / norm, c * norm
            out[s, :, i] = a
            r -= a[:, None] * c[None, :]
    return out


_LANE = np.arange(64)


def wave_sum(lanes) -> np.ndarray:
    """The wave's butterfly sum of 64 lane values (the last axis, [..., 64]): every lane adds its partner lane ^ 32, then
    ^ 16, 8, 4, 2, 1 -- the order of the device's wave_sum.  Returns lane 0's total (all lanes hold the same bits)."""
    x = np.asarray(lanes, dtype=np.float64)
    if x.shape[-1] != 64:
        raise ValueError("wave_sum: 64 lanes on the last axis")
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., _LANE ^ o]
    return x[..., 0]


def row_sum(terms) -> np.ndarray:
    """The sum of terms [..., n] along the last axis in the order of the device's row kernels (k_pixel_moments,
    k_sysrem_rows): lane l adds the terms l, l + 64, l + 128, ... in that order from +0, then wave_sum."""
    t = np.asarray(terms, dtype=np.float64)
    acc = np.zeros(t.shape[:-1] + (64,))
    for k in range(0, t.shape[-1], 64):
        chunk = t[..., k:k + 64]
        acc[..., :chunk.shape[-1]] = acc[..., :chunk.shape[-1]] + chunk
    return wave_sum(acc)


def inject_reference(pairs, obs: Observed, p0: float, p1: float) -> np.ndarray:
    """[nexp, npix]: the injected exposures of trx_detrend_observed from the pixel pairs [nexp, npix, 2] of a run and the
    RAW observed set: where b > 0, g = gain_p * (a / b), m = p0 * g, m = m + p1, f0 = F * m; F's bits elsewhere."""
    g, on = _model(pairs, obs)
    m = np.float64(p0) * g
    m = m + np.float64(p1)
    return np.where(on, obs.data * m, obs.data)


def _ratio(num, den):
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def sysrem_reference(data, weight, seg_first, ncomp: int, niter: int = 10):
    """(basis [nseg, nexp, ncomp], coef [ncomp, npix], resid [nexp, npix]): SYSREM per segment as trx_detrend_observed
    defines it (include/transit_hip.h), in numpy double in exactly its order -- the mirror of k_sysrem_cols,
    k_sysrem_rows, k_sysrem_close and k_sysrem_subtract, bit for bit.  The column sums run over v ascending, the row sums
    are row_sum's, the norm's sum runs over v ascending and its root is np.sqrt.  sysrem_basis is the same algorithm with
    numpy's own summation order."""
    resid = np.array(data, dtype=np.float64)
    if resid.ndim != 2:
        raise ValueError("sysrem_reference: data of shape [nexp][npix]")
    w_all = np.ones_like(resid) if weight is None else np.asarray(weight, dtype=np.float64)
    seg = np.asarray(seg_first, dtype=np.int64).reshape(-1)
    nexp, npix, nseg = resid.shape[0], resid.shape[1], seg.size - 1
    basis, coef = np.zeros((nseg, nexp, ncomp)), np.zeros((ncomp, npix))
    with np.errstate(all="ignore"):
        for s in range(nseg):
            k = slice(int(seg[s]), int(seg[s + 1]))
            r, w = resid[:, k], w_all[:, k]
            n = r.shape[1]
            if n == 0:
                continue
            for i in range(ncomp):
                a, c = np.ones(nexp), np.zeros(n)
                for _ in range(niter):
                    num, den = np.zeros(n), np.zeros(n)
                    for v in range(nexp):
                        num = num + (w[v] * r[v]) * a[v]
                        den = den + (w[v] * a[v]) * a[v]
                    c = _ratio(num, den)
                    a = _ratio(row_sum((w * r) * c[None, :]), row_sum((w * c[None, :]) * c[None, :]))
                n2 = np.float64(0.0)
                for v in range(nexp):
                    n2 = n2 + a[v] * a[v]
                t = np.sqrt(n2)
                if t > 0:
                    a, c = a / t, c * t
                basis[s, :, i] = a
                coef[i, k] = c
                r -= a[:, None] * c[None, :]
    return basis, coef, resid


def jacobi_rounds(nexp: int):
    """The rounds of one Jacobi sweep of trx_pca_observed over nexp exposures: the circle tournament of m = nexp rounded
    up to even, round t = 0 .. m-2 holding the pair (m-1, t) and, for k = 1 .. m/2-1, ((t+k) mod (m-1), (t-k) mod (m-1)),
    each ordered p < q, the pairs with q >= nexp (the dummy's) dropped.  A list of m - 1 lists of (p, q)."""
    nexp = int(nexp)
    if nexp < 1:
        raise ValueError("jacobi_rounds: nexp >= 1")
    m = nexp + (nexp & 1)
    rounds = []
    for t in range(m - 1):
        pairs = [(m - 1, t)] + [((t + k) % (m - 1), (t - k) % (m - 1)) for k in range(1, m // 2)]
        pairs = [(min(a, b), max(a, b)) for a, b in pairs]
        rounds.append([(p, q) for p, q in pairs if q < nexp])
    return rounds


def _jacobi(G, nsweep: int, rounds):
    """(A, V) after nsweep sweeps of the parallel-order Jacobi of trx_pca_observed on the symmetric G: every rotation of a
    round takes its parameters from A as the round finds it, then the column phase (A and V), then the row phase (A)."""
    A, V = G.copy(), np.eye(G.shape[0])
    for _ in range(nsweep):
        for pairs in rounds:
            if not pairs:
                continue
            P, Q = np.array([p for p, _ in pairs]), np.array([q for _, q in pairs])
            apq = A[P, Q]
            on = apq != 0
            if not on.any():
                continue
            P, Q, apq = P[on], Q[on], apq[on]
            theta = (A[Q, Q] - A[P, P]) / (2.0 * apq)
            t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            for M in (A, V):
                x, y = M[:, P].copy(), M[:, Q].copy()
                M[:, P] = c * x - s * y
                M[:, Q] = s * x + c * y
            x, y = A[P, :].copy(), A[Q, :].copy()
            A[P, :] = c[:, None] * x - s[:, None] * y
            A[Q, :] = s[:, None] * x + c[:, None] * y
            A[P, Q] = 0.0
            A[Q, P] = 0.0
    return A, V


def pca_reference(data, weight, seg_first, ncomp: int, nsweep: int = 8):
    """(basis [nseg, nexp, ncomp], coef [ncomp, npix], resid [nexp, npix], eigen [nseg, ncomp], offdiag [nseg], nwhole
    [nseg] int64): the principal components in time per segment as trx_pca_observed defines them (include/transit_hip.h),
    in numpy double in exactly its order -- the mirror of k_pca_live, k_pca_whole, k_pca_gram, k_pca_jacobi and
    k_pca_project, bit for bit.  An exposure is live in a segment if any of its weights there is > 0, a column whole if
    every live exposure's weight on it is; the Gram matrix of the whole columns' live entries is summed by row_sum, its
    eigenvectors come from nsweep sweeps of jacobi_rounds, ranked by descending eigenvalue (ties by ascending index; one that is not > 0 and finite ranks as 0), the
    entry of largest magnitude (the first on ties) made positive; an eigenvalue not > 0 or not finite gives the zero
    vector.  The coefficients are sums over v ascending of U * y (y the data where W > 0, +0 elsewhere) on EVERY column,
    the residuals f0 minus the components in ascending order."""
    resid = np.array(data, dtype=np.float64)
    if resid.ndim != 2:
        raise ValueError("pca_reference: data of shape [nexp][npix]")
    w_all = np.ones_like(resid) if weight is None else np.asarray(weight, dtype=np.float64)
    seg = np.asarray(seg_first, dtype=np.int64).reshape(-1)
    nexp, npix, nseg = resid.shape[0], resid.shape[1], seg.size - 1
    if not 0 <= ncomp <= nexp:
        raise ValueError("pca_reference: ncomp in 0 .. nexp")
    basis, coef = np.zeros((nseg, nexp, ncomp)), np.zeros((ncomp, npix))
    eigen, offdiag, nwhole = np.zeros((nseg, ncomp)), np.zeros(nseg), np.zeros(nseg, dtype=np.int64)
    rounds = jacobi_rounds(nexp)
    upper = np.triu_indices(nexp, 1)
    with np.errstate(all="ignore"):
        for s in range(nseg):
            k = slice(int(seg[s]), int(seg[s + 1]))
            f0, on = resid[:, k], w_all[:, k] > 0
            live = on.any(axis=1)
            whole = on[live].all(axis=0) & live.any()
            nwhole[s] = int(np.count_nonzero(whole))
            x = np.where(whole[None, :] & live[:, None], f0, 0.0)
            G = row_sum(x[:, None, :] * x[None, :, :])
            A, V = _jacobi(G, nsweep, rounds)
            lam = np.diagonal(A).copy()
            off = np.abs(A[upper])
            off = off[~np.isnan(off)]
            offdiag[s] = off.max() if off.size else 0.0
            valid = (lam > 0) & np.isfinite(lam)
            order = np.argsort(-np.where(valid, lam, 0.0), kind="stable")
            for i in range(ncomp):
                j = int(order[i])
                if not valid[j]:
                    continue
                col = V[:, j]
                if col[int(np.argmax(np.abs(col)))] < 0:
                    col = 0.0 - col                                  # (a zero entry stays +0)
                basis[s, :, i], eigen[s, i] = col, lam[j]
            U = basis[s]
            y = np.where(on, f0, 0.0)
            c = np.zeros((ncomp, f0.shape[1]))
            for v in range(nexp):
                c = c + U[v][:, None] * y[v][None, :]
            coef[:, k] = c
            for i in range(ncomp):
                f0 -= U[:, i][:, None] * c[i][None, :]
    return basis, coef, resid, eigen, offdiag, nwhole


SCATTER_NONE, SCATTER_VARIANCE, SCATTER_MASK = 0, 1, 2    # TRX_SCATTER_*: the kinds of trx_weigh_observed


def scatter_reference(data, weight, seg_first, kind: int, clip: float = 0.0, min_live: int = 2):
    """(var [npix], med [nseg], keep [npix] bool, w' [nexp, npix]): the column-scatter weights as trx_weigh_observed
    defines them (include/transit_hip.h), in numpy double in exactly its order -- the mirror of k_scatter_cols,
    k_scatter_median and k_scatter_weights, bit for bit.  data: the data installed (the residuals of a detrend, or the raw
    set); weight: the weights as set_observed installed them, None = all 1.  Per column over the entries with W > 0, v
    ascending: n, s = sum r, mean = s / n, q = sum (r - mean)^2, var = q / (n - 1) where n >= min_live and var is positive
    and finite, else +0 (dead).  med: the lower median of a segment's live var (rank (m - 1) // 2, ascending var, ties by
    ascending pixel; +0 without a live column).  keep: live and (clip == 0 or var <= (clip * clip) * med).  w': kind
    SCATTER_VARIANCE: 1 / var where W > 0 and kept; SCATTER_MASK: W where kept; +0 elsewhere.  The live columns the clip
    removed (nmasked) are (var > 0) & ~keep."""
    r = np.asarray(data, dtype=np.float64)
    if r.ndim != 2:
        raise ValueError("scatter_reference: data of shape [nexp][npix]")
    if kind not in (SCATTER_VARIANCE, SCATTER_MASK):
        raise ValueError("scatter_reference: kind SCATTER_VARIANCE or SCATTER_MASK")
    W = np.ones_like(r) if weight is None else np.asarray(weight, dtype=np.float64)
    seg = np.asarray(seg_first, dtype=np.int64).reshape(-1)
    nexp, npix, nseg = r.shape[0], r.shape[1], seg.size - 1
    on = W > 0
    with np.errstate(all="ignore"):
        n, s = np.zeros(npix, dtype=np.int64), np.zeros(npix)
        for v in range(nexp):
            n = n + on[v]
            s = np.where(on[v], s + r[v], s)
        enough = n >= min_live
        mean = s / np.where(enough, n, 1).astype(np.float64)
        q = np.zeros(npix)
        for v in range(nexp):
            d = r[v] - mean
            q = np.where(on[v], q + d * d, q)
        var = q / np.where(enough, n - 1, 1).astype(np.float64)
        var = np.where(enough & (var > 0) & np.isfinite(var), var, 0.0)
        live = var > 0
        med = np.zeros(nseg)
        for k in range(nseg):
            a, b = int(seg[k]), int(seg[k + 1])
            x = var[a:b][live[a:b]]                                  # (in ascending pixel order)
            if x.size:
                med[k] = x[np.argsort(x, kind="stable")[(x.size - 1) // 2]]
        lim = np.float64(clip) * np.float64(clip)
        lim = lim * np.repeat(med, np.diff(seg))
        keep = live & ((clip == 0) | (var <= lim))
        inv = 1.0 / np.where(keep, var, 1.0)
    if kind == SCATTER_VARIANCE:
        out = np.where(on & keep[None, :], inv[None, :], 0.0)
    else:
        out = np.where(keep[None, :], W, 0.0)
    return var, med, keep, out


NORM_ROW_NONE, NORM_ROW_QUANTILE = 0, 1                                                # TRX_NORM_ROW_*
NORM_COL_NONE, NORM_COL_DIVIDE, NORM_COL_RATIO, NORM_COL_SUBTRACT = 0, 1, 2, 3         # TRX_NORM_COL_*


@dataclass
class Normalise:
    """One trx_normalise, the recipe of step 1b of the detrending calls: row_kind NORM_ROW_NONE or NORM_ROW_QUANTILE (every
    (exposure, segment) row divided by its quantile; 0.5: the lower median), col_kind NORM_COL_NONE, _DIVIDE (f / c, about
    1), _RATIO (f / c - 1, about 0) or _SUBTRACT (f - c, about 0) with c the column's mean in time, clip 0 (none) or >= 1:
    entries beyond clip sigma of their column are replaced by the column's mean."""
    row_kind: int
    col_kind: int
    quantile: float = 0.5
    clip: float = 0.0

    def to_c(self):
        """The trx_normalise of the recipe."""
        return _abi.TrxNormalise(int(self.row_kind), int(self.col_kind), float(self.quantile), float(self.clip))


def normalise_reference(f0, weight, seg_first, nm: Normalise):
    """(data [nexp, npix], rowscale [nexp, nseg], centre [npix], nclipped, nbad): step 1b as trx_set_normalise defines it
    (include/transit_hip.h), in numpy double in exactly its order -- the mirror of k_norm_rowscale and k_norm_cols, bit for
    bit.  f0: the raw or the injected data; weight: the weights as set_observed installed them, None = all 1.  The row scale
    is the entry of rank floor(quantile * (m - 1)) of a FULL SORT of the row's m live values (np.sort: not the device's
    bisection); a row is good if m >= 1 and its scale is > 0 (+0 otherwise; 1.0 with NORM_ROW_NONE).  Per column over the
    entries live in a good row, v ascending: n, s = sum f1, c = s / n; good as the column kind asks; f2 by the kind; with a
    clip the mean and the squares of f2 about it in scatter_reference's arithmetic, an entry with d * d > (clip * clip) *
    var replaced by the mean.  Dead entries, bad rows and bad columns are +0; nbad counts the live ones among them."""
    f0 = np.asarray(f0, dtype=np.float64)
    if f0.ndim != 2:
        raise ValueError("normalise_reference: data of shape [nexp][npix]")
    if nm.row_kind not in (NORM_ROW_NONE, NORM_ROW_QUANTILE) or nm.col_kind not in (NORM_COL_NONE, NORM_COL_DIVIDE, NORM_COL_RATIO, NORM_COL_SUBTRACT):
        raise ValueError("normalise_reference: unknown row_kind or col_kind")
    if not (0.0 <= nm.quantile <= 1.0) or not (nm.clip == 0 or (nm.clip >= 1 and math.isfinite(nm.clip))):
        raise ValueError("normalise_reference: quantile in [0, 1], clip 0 or >= 1")
    W = np.ones_like(f0) if weight is None else np.asarray(weight, dtype=np.float64)
    seg = np.asarray(seg_first, dtype=np.int64).reshape(-1)
    nexp, npix, nseg = f0.shape[0], f0.shape[1], seg.size - 1
    live = W > 0
    scale = np.zeros((nexp, nseg))
    for v in range(nexp):
        for s in range(nseg):
            a, b = int(seg[s]), int(seg[s + 1])
            x = f0[v, a:b][live[v, a:b]]
            if x.size == 0:
                continue
            if nm.row_kind == NORM_ROW_NONE:
                scale[v, s] = 1.0
                continue
            k = int(np.floor(np.float64(nm.quantile) * np.float64(x.size - 1)))
            q = np.sort(x)[k]
            scale[v, s] = q if q > 0 else 0.0
    col_scale = np.repeat(scale, np.diff(seg), axis=1)                # [nexp, npix]: every entry's row scale
    on = live & (col_scale > 0)
    with np.errstate(all="ignore"):
        f1 = f0 / np.where(on, col_scale, 1.0) if nm.row_kind == NORM_ROW_QUANTILE else f0
        n, s = np.zeros(npix, dtype=np.int64), np.zeros(npix)
        for v in range(nexp):
            n = n + on[v]
            s = np.where(on[v], s + f1[v], s)
        c = s / np.where(n >= 1, n, 1).astype(np.float64)
        if nm.col_kind == NORM_COL_NONE:
            good = n >= 1
        elif nm.col_kind == NORM_COL_SUBTRACT:
            good = (n >= 1) & np.isfinite(c)
        else:
            good = (n >= 1) & (c > 0) & np.isfinite(c)
        c = np.where(good, c, 0.0)
        safe = np.where(good, c, 1.0)
        if nm.col_kind == NORM_COL_DIVIDE:
            f2 = f1 / safe[None, :]
        elif nm.col_kind == NORM_COL_RATIO:
            t = f1 / safe[None, :]
            f2 = t - 1.0
        elif nm.col_kind == NORM_COL_SUBTRACT:
            f2 = f1 - c[None, :]
        else:
            f2 = f1
        keep = on & good[None, :]
        nclipped = 0
        if nm.clip > 0:
            clips = good & (n >= 2)
            s2 = np.zeros(npix)
            for v in range(nexp):
                s2 = np.where(keep[v], s2 + f2[v], s2)
            mean = s2 / np.where(clips, n, 1).astype(np.float64)
            q = np.zeros(npix)
            for v in range(nexp):
                d = f2[v] - mean
                q = np.where(keep[v], q + d * d, q)
            var = q / np.where(clips, n - 1, 1).astype(np.float64)
            lim = np.float64(nm.clip) * np.float64(nm.clip)
            lim = lim * var
            d = f2 - mean[None, :]
            hit = keep & clips[None, :] & (d * d > lim[None, :])
            nclipped = int(np.count_nonzero(hit))
            f2 = np.where(hit, mean[None, :], f2)
    data = np.where(keep, f2, 0.0)
    return data, scale, c, nclipped, int(np.count_nonzero(live & ~keep))


def _check_wfilter(obs: Observed, wf: WeightedFilter):
    if (wf.nseg, wf.nexp) != (obs.nseg, obs.nexp):
        raise ValueError("weighted filter of the observed set's nseg and nexp")


def _wf_factor(obs: Observed, wf: WeightedFilter, dtype):
    """(L [n, n, npix], D [n, npix], N_jj [n, npix]): the definition's install step in `dtype`, vectorised over the
    columns, every operation in its order"""
    _check_wfilter(obs, wf)
    n, npix = wf.ncomp, obs.npix
    w = (obs.weight if obs.weight is not None else np.ones_like(obs.data)).astype(dtype)
    N = np.zeros((n, n, npix), dtype=dtype)
    for s in range(obs.nseg):
        k = slice(int(obs.seg_first[s]), int(obs.seg_first[s + 1]))
        U = wf.basis[s].astype(dtype)
        for j in range(n):
            for i in range(j + 1):
                acc = np.zeros(k.stop - k.start, dtype=dtype)
                for v in range(obs.nexp):
                    acc = acc + (U[v, j] * w[v, k]) * U[v, i]
                N[j, i, k] = acc
    T, L, D = np.zeros_like(N), np.zeros_like(N), np.zeros((n, npix), dtype=dtype)
    with np.errstate(all="ignore"):
        for j in range(n):
            for i in range(j):
                t = N[j, i].copy()
                for m in range(i):
                    t = t - T[j, m] * L[i, m]
                T[j, i] = t
                L[j, i] = t / D[i]
            d = N[j, j].copy()
            for i in range(j):
                d = d - T[j, i] * L[j, i]
            D[j] = d
    return L, D, np.stack([N[j, j] for j in range(n)]) if n else np.zeros((0, npix), dtype=dtype)


def _wf_fit(g, obs: Observed, wf: WeightedFilter, L, D, dtype, live=None):
    """(c [n, npix], g' [nexp, npix]) in `dtype` from g: the definition's run step, vectorised over the columns -- the
    coefficients of every column's solve and g less their combination of the vectors.  live [npix] (trx_regress_observed):
    a column where it is False gets the coefficients +0, its solve's result unused"""
    n = wf.ncomp
    w = (obs.weight if obs.weight is not None else np.ones_like(obs.data)).astype(dtype)
    g = g.astype(dtype)
    out, coef = np.zeros(g.shape, dtype=dtype), np.zeros((n, g.shape[1]), dtype=dtype)
    with np.errstate(all="ignore"):
        for s in range(obs.nseg):
            k = slice(int(obs.seg_first[s]), int(obs.seg_first[s + 1]))
            U = wf.basis[s].astype(dtype)
            y = []
            for j in range(n):
                acc = np.zeros(k.stop - k.start, dtype=dtype)
                for v in range(obs.nexp):
                    acc = acc + (U[v, j] * w[v, k]) * g[v, k]
                y.append(acc)
            z = []
            for j in range(n):
                t = np.zeros(k.stop - k.start, dtype=dtype)
                for i in range(j):
                    t = t + L[j, i, k] * z[i]
                z.append(y[j] - t)
            q = [z[j] / D[j, k] for j in range(n)]
            c = [None] * n
            for j in range(n - 1, -1, -1):
                t = np.zeros(k.stop - k.start, dtype=dtype)
                for i in range(j + 1, n):
                    t = t + L[i, j, k] * c[i]
                c[j] = q[j] - t
            for j in range(n):
                if live is not None:
                    c[j] = np.where(live[k], c[j], dtype(0.0))
                coef[j, k] = c[j]
            for v in range(obs.nexp):
                r = np.zeros(k.stop - k.start, dtype=dtype)
                for j in range(n):
                    r = r + U[v, j] * c[j]
                out[v, k] = g[v, k] - r
    return coef, out


def _wf_apply(g, obs: Observed, wf: WeightedFilter, L, D, dtype):
    """g' [nexp, npix] in `dtype` from g: the definition's run step, vectorised over the columns"""
    return _wf_fit(g, obs, wf, L, D, dtype)[1]


def weighted_pivots(obs: Observed, wf: WeightedFilter) -> np.ndarray:
    """[npix, ncomp]: every pivot's share D_j / N_jj of its diagonal entry in the mirror (nan for N_jj = 0): a pivot is
    singular when this is not above _abi.WFILTER_PIVOT"""
    _, D, njj = _wf_factor(obs, wf, np.float64)
    with np.errstate(all="ignore"):
        return (D / njj).T


def weighted_factor(obs: Observed, wf: WeightedFilter):
    """(L [npix, ncomp, ncomp], D [npix, ncomp], live [npix]): every column's factor of trx_set_weighted_filter, the
    definition's install step in numpy double in exactly its order -- the mirror of k_wfilter_factor, bit for bit.  L is
    strictly lower triangular (the unit diagonal is implied); live: no pivot of the column is singular,
    D_j > 2^-26 N_jj for every j.  What follows a singular pivot in L and D is whatever the arithmetic gives."""
    L, D, njj = _wf_factor(obs, wf, np.float64)
    with np.errstate(all="ignore"):
        live = np.all(D > _abi.WFILTER_PIVOT * njj, axis=0) if wf.ncomp else np.ones(obs.npix, dtype=bool)
    return np.ascontiguousarray(L.transpose(2, 0, 1)), np.ascontiguousarray(D.T), live


def weighted_filter_reference(pairs, obs: Observed, wf: WeightedFilter) -> np.ndarray:
    """g' [nexp, npix] of the weighted filter from the pixel pairs [nexp, npix, 2] of a run: the definition's run step in
    numpy double in exactly its order, from weighted_factor's factor -- the mirror of k_pixel_wfilter, bit for bit.  A
    column with b <= 0 at any exposure or with a singular pivot is NaN.  How far it can lie from the exact projection of
    the same g: weighted_filter_bound."""
    g, on = _model(pairs, obs)
    L, D, live = weighted_factor(obs, wf)
    out = _wf_apply(g, obs, wf, L.transpose(1, 2, 0), D.T, np.float64)
    return np.where((live & np.all(on, axis=0))[None, :], out, np.nan)


def weighted_filter_bound(pairs, obs: Observed, wf: WeightedFilter) -> np.ndarray:
    """[nexp, npix]: how far a double evaluation of the definition (weighted_filter_reference, the device) can lie from
    the exact weighted projection of the same g (weighted_filter_exact stands for it), NaN in the dead columns.  For one
    column, with u = 2^-53, n = ncomp, N = U^T diag(w) U, y = U^T diag(w) g, c = N^-1 y, |.| taken entry by entry, to
    first order in u:

      - y_j: every term is two products, and nexp of them are added from +0:
            |dy_j| <= (nexp + 1) u Ya_j,          Ya_j = sum_v |U_vj| w_v |g_v|;
        in the same way |dN_jk| <= (nexp + 1) u Na_jk, Na_jk = sum_v |U_vj| w_v |U_vk|;
      - the factor and the two triangular solves: the computed c solves (N + dN + E) c = y + dy with
        |E| <= (3 n + 1) u |L| |D| |L^T|, the bound of a Cholesky solve (Higham, Accuracy and Stability of Numerical
        Algorithms, theorems 10.3 and 10.4; with R = D^1/2 L^T this is |R^T| |R|: a row of the factor takes at most n
        products and a division, each solve as many), and by Cauchy-Schwarz over the columns of R
            (|R^T| |R|)_jk <= S_jk = sqrt(N_jj N_kk);
      - so |dc| <= |N^-1| ((nexp + 1) u Ya + ((nexp + 1) u Na + (3 n + 1) u S) |c|);
      - r_v = sum_j U_vj c_j, n products added from +0, and one subtraction:
            |dg'_v| <= sum_j |U_vj| |dc_j| + n u sum_j |U_vj| |c_j| + u |g'_v|.

    Doubled, for the terms of second order (the pivot rule keeps N far from singular in a live column).  N^-1 and c are
    taken from numpy's inverse in double, whose own error is of second order here."""
    _check_wfilter(obs, wf)
    g, on = _model(pairs, obs)
    live = weighted_factor(obs, wf)[2] & np.all(on, axis=0)
    w = obs.weight if obs.weight is not None else np.ones_like(obs.data)
    n, nexp, u = wf.ncomp, obs.nexp, 2.0 ** -53
    out = np.full(g.shape, np.nan)
    for s in range(obs.nseg):
        k = np.arange(obs.seg_first[s], obs.seg_first[s + 1])
        k = k[live[k]]
        if k.size == 0:
            continue
        U, aU = wf.basis[s], np.abs(wf.basis[s])
        N = np.einsum("vj,vp,vi->pji", U, w[:, k], U)
        Na = np.einsum("vj,vp,vi->pji", aU, w[:, k], aU)
        y, Ya = np.einsum("vj,vp->pj", U, w[:, k] * g[:, k]), np.einsum("vj,vp->pj", aU, w[:, k] * np.abs(g[:, k]))
        Ninv = np.linalg.inv(N)
        c = np.einsum("pji,pi->pj", Ninv, y)
        d = np.sqrt(np.einsum("pjj->pj", N))
        S = d[:, :, None] * d[:, None, :]
        rhs = (nexp + 1) * u * Ya + np.einsum("pji,pi->pj", (nexp + 1) * u * Na + (3 * n + 1) * u * S, np.abs(c))
        dc = np.einsum("pji,pi->pj", np.abs(Ninv), rhs)
        gp = g[:, k] - U @ c.T
        out[:, k] = 2.0 * (aU @ dc.T + n * u * (aU @ np.abs(c).T) + u * np.abs(gp))
    return out


def weighted_filter_exact(pairs, obs: Observed, wf: WeightedFilter) -> np.ndarray:
    """The same least-squares projection with the factor and the solve in np.longdouble, rounded to double at the end; g
    as the moments take it, the dead columns (NaN) the mirror's."""
    g, on = _model(pairs, obs)
    live = weighted_factor(obs, wf)[2] & np.all(on, axis=0)
    L, D, _ = _wf_factor(obs, wf, np.longdouble)
    out = _wf_apply(g, obs, wf, L, D, np.longdouble).astype(np.float64)
    return np.where(live[None, :], out, np.nan)


def regress_reference(f0, weight, seg_first, vectors):
    """(coef [nvec, npix], resid [nexp, npix], nsingular): every pixel column of f0 [nexp, npix] regressed on its segment's
    time vectors ([nseg, nexp, nvec], or [nexp, nvec] for all segments) by weighted least squares under its own weights
    (None: all 1), as trx_regress_observed defines it (include/transit_hip.h) -- the mirror of k_wfilter_factor and
    k_regress_cols, bit for bit.  It is the weighted filter's install and run steps (_wf_factor, _wf_fit) with g = f0: a
    column with a singular pivot gets the coefficients +0 and keeps f0; nsingular counts them."""
    f0 = np.ascontiguousarray(f0, dtype=np.float64)
    if f0.ndim != 2:
        raise ValueError("regress_reference: f0 of shape [nexp][npix]")
    seg = np.asarray(seg_first, dtype=np.int64).reshape(-1)
    vec = np.asarray(vectors, dtype=np.float64)
    if vec.ndim == 2:
        vec = np.broadcast_to(vec[None, :, :], (seg.size - 1,) + vec.shape)
    if vec.ndim != 3 or vec.shape[:2] != (seg.size - 1, f0.shape[0]) or not np.isfinite(vec).all():
        raise ValueError("regress_reference: finite vectors of shape [nseg][nexp][nvec] or [nexp][nvec]")
    obs, wf = Observed(seg, f0, weight), WeightedFilter(vec)
    L, D, njj = _wf_factor(obs, wf, np.float64)
    with np.errstate(all="ignore"):
        live = np.all(D > _abi.WFILTER_PIVOT * njj, axis=0) if wf.ncomp else np.ones(obs.npix, dtype=bool)
    coef, resid = _wf_fit(f0, obs, wf, L, D, np.float64, live)
    return coef, resid, int(np.count_nonzero(~live))


def time_basis(x, degree: int) -> np.ndarray:
    """[nexp, degree + 1]: the powers 0 .. degree of t = (x - mean(x)) / max|x - mean(x)| -- of the airmass of every
    exposure, say --, a well-conditioned set of vectors for regress_reference and Engine.regress_observed (a constant x
    gives t = 0).  A convenience: the call takes any finite vectors."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if degree < 0 or not np.isfinite(x).all():
        raise ValueError("time_basis: finite x and degree >= 0")
    d = x - np.mean(x)
    span = np.max(np.abs(d)) if d.size else 0.0
    t = d / span if span > 0 else np.zeros_like(d)
    return np.stack([t ** k for k in range(degree + 1)], axis=1)


def filtered_map_reference(pairs_at_lags, obs: Observed, filt, vm: VelocityMap) -> np.ndarray:
    """The definition of trx_run_filtered_map in numpy: the map [nkp, nvsys] from the pixel pairs [nlag, npix, 2] of
    run_pixels at vm.lag.  Cell (i, j) takes at exposure v the row nearest_lags(vm)[i, j, v]; that matrix goes through
    filter_reference (a WeightedFilter: weighted_filter_reference) and reference_values as a filtered run's does, and
    cell_value gives the cell.  A cell with a
    velocity outside the lag grid is nan.  (With a high-pass: highpass_pairs of highpass_reference of the pairs, and a
    gain-free copy of the observed set.)"""
    values = weighted_filter_reference if isinstance(filt, WeightedFilter) else filter_reference
    pairs = np.asarray(pairs_at_lags, dtype=np.float64)
    if pairs.shape != (vm.nlag, obs.npix, 2):
        raise ValueError("pairs of shape [nlag][npix][2] with the map's nlag")
    if vm.nexp != obs.nexp:
        raise ValueError("a map of the observed set's nexp")
    idx = nearest_lags(vm)
    out = np.full((vm.nkp, vm.nvsys), np.nan)
    for i in range(vm.nkp):
        for j in range(vm.nvsys):
            if np.all(idx[i, j] >= 0):
                out[i, j] = cell_value(reference_values(values(pairs[idx[i, j]], obs, filt), obs), vm)
    return out


def exposed_map_rows(vm: VelocityMap):
    """(lo, hi, base, R) of trx_run_exposed_map: over the cells inside the lag grid, per exposure v the least and the largest
    lag the cells take (lo[v], hi[v]; 2^31 - 1 and -1 where no cell is inside), base[v] = n_0 + ... + n_{v-1} with
    n_v = hi[v] - lo[v] + 1 (0 for such an exposure), and R the sum of the n_v: the pixel rows the call makes, row
    base[v] + (l - lo[v]) the pair (lag l, exposure v)."""
    idx = nearest_lags(vm).reshape(-1, vm.nexp)
    idx = idx[np.all(idx >= 0, axis=1)]
    if idx.shape[0] == 0:
        lo, hi = np.full(vm.nexp, 2 ** 31 - 1, dtype=np.int64), np.full(vm.nexp, -1, dtype=np.int64)
    else:
        lo, hi = idx.min(axis=0).astype(np.int64), idx.max(axis=0).astype(np.int64)
    n = np.where(hi >= lo, hi - lo + 1, 0)
    base = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    return lo, hi, base, int(np.sum(n))


def exposed_map_reference(pairs_lv, obs: Observed, filt, vm: VelocityMap, hp=None) -> np.ndarray:
    """The definition of trx_run_exposed_map in numpy: the map [nkp, nvsys] from pairs_lv [nlag, nexp, npix, 2], with
    pairs_lv[l][v] the pair row run_exposed gives for exposure v at the shift vm.lag[l] (the table's scale and smear in
    it).  Cell (i, j) takes at exposure v the row pairs_lv[nearest_lags(vm)[i, j, v], v]; that matrix goes through the
    high-pass when one is given (highpass_pairs of highpass_reference, and a gain-free copy of the observed set from
    there on), filter_reference (a WeightedFilter: weighted_filter_reference) and reference_values as a filtered run's
    does, and cell_value gives the cell.  A cell with a velocity outside the lag grid is nan."""
    values = weighted_filter_reference if isinstance(filt, WeightedFilter) else filter_reference
    pairs = np.asarray(pairs_lv, dtype=np.float64)
    if pairs.shape != (vm.nlag, obs.nexp, obs.npix, 2):
        raise ValueError("pairs of shape [nlag][nexp][npix][2] with the map's nlag")
    if vm.nexp != obs.nexp:
        raise ValueError("a map of the observed set's nexp")
    behind = Observed(obs.seg_first, obs.data, obs.weight) if hp is not None else obs
    idx = nearest_lags(vm)
    ve = np.arange(obs.nexp)
    out = np.full((vm.nkp, vm.nvsys), np.nan)
    for i in range(vm.nkp):
        for j in range(vm.nvsys):
            if np.all(idx[i, j] >= 0):
                m = pairs[idx[i, j], ve]
                if hp is not None:
                    m = highpass_pairs(highpass_reference(m, obs, hp))
                out[i, j] = cell_value(reference_values(values(m, behind, filt), behind), vm)
    return out


@dataclass
class HighPass:
    """One trx_highpass: the symmetric tap table taps[0 .. half] (finite, >= 0, taps[0] > 0), taps[k] the weight at a
    distance of k pixels."""
    taps: np.ndarray

    def __post_init__(self):
        self.taps = np.ascontiguousarray(self.taps, dtype=np.float64).reshape(-1)
        if self.taps.size < 1:
            raise ValueError("HighPass: at least taps[0]")

    @property
    def half(self) -> int:
        return int(self.taps.size) - 1

    def to_c(self):
        """The trx_highpass of the table (the array stays owned by this object)."""
        c = _abi.TrxHighpass()
        c.half, c.pad = self.half, 0
        c.taps = self.taps.ctypes.data_as(_abi.c_double_p)
        return c


def gaussian_highpass(sigma_pix: float, cut: float = 3.0) -> HighPass:
    """A running Gaussian mean of sigma_pix pixels cut at cut sigmas: taps exp(-k^2 / (2 sigma^2)), half = floor(cut * sigma)."""
    if not (sigma_pix > 0) or not (cut > 0):
        raise ValueError("gaussian_highpass: sigma_pix > 0 and cut > 0")
    k = np.arange(int(math.floor(cut * sigma_pix)) + 1, dtype=np.float64)
    return HighPass(np.exp(-(k * k) / (2.0 * sigma_pix * sigma_pix)))


def boxcar_highpass(width: int) -> HighPass:
    """A running mean over width pixels (odd): width equal taps, half = (width - 1) / 2."""
    if width < 1 or width % 2 != 1:
        raise ValueError("boxcar_highpass: an odd width >= 1")
    return HighPass(np.ones((width - 1) // 2 + 1))


def highpass_reference(pairs, obs: Observed, hp: HighPass) -> np.ndarray:
    """The definition: g' [n, npix] from the pixel pairs [n, npix, 2] of a run at n shifts (or lags), the observed set's
    segments and gain, and the taps -- vectorised over the pixels with a loop over k = -half .. half; a skipped term (its
    pixel outside the segment or dead) is added as taps * 0, which leaves a sum that started from +0 as it is, bit for
    bit.  NaN where the pixel is dead.  Engine.run_highpassed gives these bits."""
    pairs = np.asarray(pairs, dtype=np.float64)
    if pairs.ndim != 3 or pairs.shape[1:] != (obs.npix, 2):
        raise ValueError("pairs of shape [n][npix][2]")
    a, b = pairs[..., 0], pairs[..., 1]
    gain = obs.gain if obs.gain is not None else np.ones(obs.npix)
    on = b > 0
    with np.errstate(all="ignore"):
        g = np.where(on, gain[None, :] * (a / np.where(on, b, 1.0)), 0.0)
    live = on.astype(np.float64)
    out = np.full(g.shape, np.nan)
    n, half = g.shape[0], hp.half
    for s in range(obs.nseg):
        first, last = int(obs.seg_first[s]), int(obs.seg_first[s + 1])
        if last <= first:
            continue
        m = last - first
        gz, lz = np.zeros((n, m + 2 * half)), np.zeros((n, m + 2 * half))
        gz[:, half:half + m], lz[:, half:half + m] = g[:, first:last], live[:, first:last]
        num, den = np.zeros((n, m)), np.zeros((n, m))
        with np.errstate(all="ignore"):
            for k in range(-half, half + 1):
                t = hp.taps[abs(k)]
                num = num + t * gz[:, half + k:half + k + m]
                den = den + t * lz[:, half + k:half + k + m]
            v = g[:, first:last] - num / den
        out[:, first:last] = np.where(on[:, first:last], v, np.nan)
    return out


def highpass_observed_reference(data, weight, seg_first, hp: HighPass):
    """(values [nexp, npix], ndead): the observed set's own data through the high-pass as trx_highpass_observed defines it
    (include/transit_hip.h) -- the mirror of k_data_highpass, bit for bit.  data: the data the call reads (the residuals
    of a detrend, or the raw set); weight: the weights as set_observed installed them (None: all 1).  It is
    highpass_reference of the pairs (data, weight > 0) without a gain -- g = 1 * (r / 1) is r --, with +0 in place of NaN
    at the dead entries; ndead is their count."""
    data = np.asarray(data, dtype=np.float64)
    if data.ndim != 2:
        raise ValueError("data of shape [nexp][npix]")
    live = np.ones(data.shape, dtype=bool) if weight is None else np.asarray(weight, dtype=np.float64) > 0
    if live.shape != data.shape:
        raise ValueError("weight of the data's shape")
    v = highpass_reference(np.stack([data, live.astype(np.float64)], axis=-1), Observed(seg_first, data, None, None), hp)
    return np.where(live, v, 0.0), int(np.count_nonzero(~live))


def highpass_pairs(values) -> np.ndarray:
    """The pairs [n, npix, 2] the device keeps of high-passed values [n, npix]: (g', 1) for a live pixel, (0, 0) for a dead
    one (NaN).  reference, trail_reference and filter_reference of them with a gain-free copy of the observed set are the
    runs with the high-pass installed."""
    values = np.asarray(values, dtype=np.float64)
    has = ~np.isnan(values)
    return np.stack([np.where(has, values, 0.0), has.astype(np.float64)], axis=-1)
