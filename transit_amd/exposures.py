"""Host side of the exposure table, Engine.set_exposures / Engine.run_exposed and their Batch forms
(trx_set_exposures / trx_run_exposed, include/transit_hip.h).

The table carries what differs from exposure to exposure in the forward model of a time series and must act before the
filter: a factor `scale[v]` on the model (the light curve, the phase function) and `smear[v]` = eta_v, the HALF-width of the
change of the planet's Doppler factor over the exposure, relative (dv / 2c).  A row with eta > 0 is the spectrum under the
box of half-width d = centre' * eta convolved with the pixel's Gaussian, W = erf((x + d) / q) - erf((x - d) / q) with
q = sigma sqrt(2), over the bins within cut * sigma + d of the centre; a row with eta == 0 is the plain pixel row.

    Exposures(scale=None, smear=None)        a table (to_c(): its trx_exposures)
    smear_half(kp_kms, phase, dphase)        eta of an exposure of length dphase at orbital phase `phase`
    exposed_range(wn_i, wn_d, nwn, centre, fwhm, cut, eta)
                                             the bins [i_lo, i_hi) of a rest-frame window, the header's rule
    reference(spec, wn_i, wn_d, nwn, px, shifts, ex, lo=0)
                                             the definition: erf weights, sums by math.fsum
    subshift_average(spec, wn_i, wn_d, nwn, px, shifts, ex, nsub)
                                             the physical cross-check: plain pixel VALUES averaged over nsub sub-shifts
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _abi, bands, pixels

SMEAR_MAX = 0.01      # TRX_SMEAR_MAX
SQRT2 = math.sqrt(2.0)

try:                    # (either is within an ulp or two of erf; scipy's takes an array at once)
    from scipy.special import erf as _erf
except ImportError:
    _erf = np.vectorize(math.erf, otypes=[np.float64])


@dataclass
class Exposures:
    """One trx_exposures: per exposure a finite factor on the model (None: 1) and a smear half-width eta in
    [0, SMEAR_MAX] (None: 0)."""
    scale: Optional[np.ndarray] = None
    smear: Optional[np.ndarray] = None

    def __post_init__(self):
        if self.scale is not None:
            self.scale = np.ascontiguousarray(self.scale, dtype=np.float64).reshape(-1)
        if self.smear is not None:
            self.smear = np.ascontiguousarray(self.smear, dtype=np.float64).reshape(-1)
        if self.scale is not None and self.smear is not None and self.scale.size != self.smear.size:
            raise ValueError("Exposures: scale and smear of the same length")

    def __len__(self) -> int:
        return int(self.scale.size if self.scale is not None else self.smear.size if self.smear is not None else 0)

    def to_c(self):
        """The trx_exposures of the table (the arrays stay owned by this object)."""
        c = _abi.TrxExposures()
        c.nexp = len(self)
        c.scale = self.scale.ctypes.data_as(_abi.c_double_p) if self.scale is not None else None
        c.smear = self.smear.ctypes.data_as(_abi.c_double_p) if self.smear is not None else None
        return c

    def eta(self, v: int) -> float:
        return float(self.smear[v]) if self.smear is not None else 0.0

    def factor(self, v: int):
        return float(self.scale[v]) if self.scale is not None else None


def smear_half(kp_kms: float, phase: float, dphase: float) -> float:
    """eta of an exposure lasting dphase (in orbital phase) at phase `phase` (0: mid-transit) of a circular orbit with
    radial-velocity semi-amplitude kp_kms: |Kp 2 pi cos(2 pi phase) dphase| / (2 c)."""
    return abs(float(kp_kms) * 2.0 * math.pi * math.cos(2.0 * math.pi * float(phase)) * float(dphase)) / (2.0 * pixels.C_KMS)


def exposed_range(wn_i: float, wn_d: float, nwn: int, centre: float, fwhm: float, cut: float, eta: float):
    """The bins [i_lo, i_hi) of the rest-frame window (centre, fwhm) = (centre_p / s, fwhm_p / s) with smear half-width
    eta, by the rule of trx_set_exposures: within cut * sigma + centre * eta of the centre, in double, clipped to [0, nwn);
    an edge that is not a number gives no bin."""
    sigma = fwhm / bands.FWHM_PER_SIGMA
    d = centre * eta if eta > 0.0 else 0.0
    r = cut * sigma + d
    a, z = (centre - r - wn_i) / wn_d, (centre + r - wn_i) / wn_d
    if a != a or z != z:
        return 0, 0
    n = float(nwn)
    a, z = math.ceil(a) if abs(a) != math.inf else a, math.floor(z) + 1.0 if abs(z) != math.inf else z
    first = 0 if a <= 0 else nwn if a >= n else int(a)
    last = 0 if z <= 0 else nwn if z >= n else int(z)
    return first, max(first, last)


def _window(wn_i, wn_d, nwn, centre, fwhm, cut, eta, lo, n):
    a, z = exposed_range(wn_i, wn_d, nwn, centre, fwhm, cut, eta)
    return max(a, lo), min(z, lo + n)


def reference(spec, wn_i: float, wn_d: float, nwn: int, px: pixels.Pixels, shifts, ex: Exposures, lo: int = 0) -> np.ndarray:
    """The definition: [nexp, npix, 2] over the spectrum `spec` of shard [lo, lo + len(spec)) -- rows with eta == 0 from
    pixels.reference, rows with eta > 0 with erf weights (scipy.special.erf, or math.erf without scipy) and sums by
    math.fsum; then a times the row's scale (a pair with no bin in the shard stays (+0, +0))."""
    spec = np.asarray(spec, dtype=np.float64)
    shifts = np.asarray(shifts, dtype=np.float64).reshape(-1)
    out = np.zeros((shifts.size, len(px), 2))
    for v, s in enumerate(shifts):
        s, eta = float(s), ex.eta(v)
        if eta > 0.0:
            for p in range(len(px)):
                centre, fwhm = float(px.centre[p]) / s, float(px.fwhm[p]) / s
                a, z = _window(wn_i, wn_d, nwn, centre, fwhm, px.cut, eta, lo, spec.size)
                if z <= a:
                    continue
                q = (fwhm / bands.FWHM_PER_SIGMA) * SQRT2
                d = centre * eta
                x = (wn_i + np.arange(a, z) * wn_d) - centre
                w = _erf((x + d) / q) - _erf((x - d) / q)
                out[v, p, 0] = math.fsum(w * spec[a - lo:z - lo])
                out[v, p, 1] = math.fsum(w)
        else:
            out[v] = pixels.reference(spec, wn_i, wn_d, nwn, px, [s], lo=lo)[0]
        c = ex.factor(v)
        if c is not None:
            nz = out[v, :, 1] != 0
            out[v, nz, 0] = c * out[v, nz, 0]
    return out


def subshift_average(spec, wn_i: float, wn_d: float, nwn: int, px: pixels.Pixels, shifts, ex: Exposures, nsub: int = 401,
                     lo: int = 0) -> np.ndarray:
    """What the smear stands for: [nexp, npix], the mean of the plain pixel VALUES (a / b of trx_run_pixels' pairs, the
    Gaussian weights over their own cut) at the nsub midpoints of the Doppler factors [s (1 - eta), s (1 + eta)], times the
    row's scale.  NaN where a sub-shift's window has no bin."""
    spec = np.asarray(spec, dtype=np.float64)
    shifts = np.asarray(shifts, dtype=np.float64).reshape(-1)
    out = np.zeros((shifts.size, len(px)))
    mid = (2.0 * (np.arange(nsub) + 0.5) / nsub - 1.0)
    for v, s in enumerate(shifts):
        sub = float(s) * (1.0 + ex.eta(v) * mid) if ex.eta(v) > 0.0 else np.array([float(s)])
        for p in range(len(px)):
            centre, sigma = float(px.centre[p]) / sub, float(px.fwhm[p]) / sub / bands.FWHM_PER_SIGMA
            a = np.clip(np.ceil((centre - px.cut * sigma - wn_i) / wn_d), lo, lo + spec.size).astype(np.int64)
            z = np.clip(np.floor((centre + px.cut * sigma - wn_i) / wn_d) + 1, lo, lo + spec.size).astype(np.int64)
            i = np.arange(int(a.min()), max(int(z.max()), int(a.min())))
            x = ((wn_i + i * wn_d)[None, :] - centre[:, None]) / sigma[:, None]
            w = np.where((i[None, :] >= a[:, None]) & (i[None, :] < z[:, None]), np.exp(-0.5 * (x * x)), 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                out[v, p] = np.mean((w @ spec[i - lo]) / w.sum(axis=1))
        c = ex.factor(v)
        if c is not None:
            out[v] *= c
    return out
