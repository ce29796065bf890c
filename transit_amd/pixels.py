"""Host side of the detector-pixel runs, Engine.set_pixels / Engine.run_pixels and their Batch forms
(trx_set_pixels / trx_run_pixels, include/transit_hip.h).

A pixel set is a detector: per pixel a centre and a line-spread FWHM, both in the OBSERVED frame, and one window
half-width `cut` in sigmas.  A run takes a list of Doppler shifts (nu_observed / nu_rest) and returns, per shift v and
pixel p, the pair (sum of w_i S_i, sum of w_i) of the band gauss(centre_p / shift_v, fwhm_p / shift_v, cut) over the
bins of the handle's shard:

    Pixels(centre, fwhm, cut=4)              a pixel set
    resolving_power(centres, R, cut=4)       fwhm = centre / R at every pixel
    shift(v_kms)                             sqrt((1 - beta) / (1 + beta)) for a source receding at v_kms
    as_bands(pixels, shifts)                 the equivalent bands.gauss list, in [v][p] order
    reference(spec, wn_i, wn_d, nwn, pixels, shifts, lo=0)
                                             the definition in numpy, sums by math.fsum
    combine(parts)                           shard partial pairs added in the order given (rank order)
    value(out)                               out[..., 0] / out[..., 1]
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import _abi, bands

C_KMS = 299792.458


@dataclass
class Pixels:
    """One trx_pixels: centres and FWHMs (cm-1, observed frame; finite and > 0, any order), cut in sigmas."""
    centre: np.ndarray
    fwhm: np.ndarray
    cut: float = 4.0

    def __post_init__(self):
        self.centre = np.ascontiguousarray(self.centre, dtype=np.float64).reshape(-1)
        self.fwhm = np.ascontiguousarray(self.fwhm, dtype=np.float64).reshape(-1)
        self.cut = float(self.cut)
        if self.centre.shape != self.fwhm.shape:
            raise ValueError("Pixels: centre and fwhm of the same length")

    def __len__(self) -> int:
        return int(self.centre.size)


def resolving_power(centres, R: float, cut: float = 4.0) -> Pixels:
    """Pixels at the given centres with fwhm = centre / R."""
    c = np.asarray(centres, dtype=np.float64)
    return Pixels(c, c / float(R), cut)


def shift(v_kms: float) -> float:
    """nu_observed / nu_rest of a source receding at v_kms (negative: approaching): the relativistic
    sqrt((1 - beta) / (1 + beta))."""
    beta = float(v_kms) / C_KMS
    return math.sqrt((1.0 - beta) / (1.0 + beta))


def to_c(px: Pixels):
    """The trx_pixels of a set (the arrays stay owned by the Pixels object)."""
    c = _abi.TrxPixels()
    c.npix = len(px)
    c.centre = px.centre.ctypes.data_as(_abi.c_double_p)
    c.fwhm = px.fwhm.ctypes.data_as(_abi.c_double_p)
    c.cut = px.cut
    return c


def as_bands(px: Pixels, shifts):
    """The bands whose sums a pixel run returns: gauss(centre_p / shift_v, fwhm_p / shift_v, cut), v outer, p inner."""
    out = []
    for s in np.asarray(shifts, dtype=np.float64).reshape(-1):
        s = float(s)
        out += [bands.gauss(float(c) / s, float(f) / s, px.cut) for c, f in zip(px.centre, px.fwhm)]
    return out


def reference(spec, wn_i: float, wn_d: float, nwn: int, px: Pixels, shifts, lo: int = 0) -> np.ndarray:
    """The definition: [nshift, npix, 2] over the spectrum `spec` of shard [lo, lo + len(spec)) of the grid
    nu_i = wn_i + i wn_d (i < nwn) -- ranges by bands.gauss_range, weights in numpy, sums by math.fsum."""
    spec = np.asarray(spec, dtype=np.float64)
    shifts = np.asarray(shifts, dtype=np.float64).reshape(-1)
    out = np.zeros((shifts.size, len(px), 2))
    for v, s in enumerate(shifts):
        s = float(s)
        for p in range(len(px)):
            centre, fwhm = float(px.centre[p]) / s, float(px.fwhm[p]) / s
            a, z = bands.gauss_range(wn_i, wn_d, nwn, centre, fwhm, px.cut)
            a, z = max(a, lo), min(z, lo + spec.size)
            if z <= a:
                continue
            i = np.arange(a, z)
            sigma = fwhm / bands.FWHM_PER_SIGMA
            x = ((wn_i + i * wn_d) - centre) / sigma
            w = np.exp(-0.5 * (x * x))
            out[v, p, 0] = math.fsum(w * spec[i - lo])
            out[v, p, 1] = math.fsum(w)
    return out


def combine(parts) -> np.ndarray:
    """Partial pairs of the shards ([nshift][npix][2] each), added in the order given -- rank order for the job's."""
    return bands.combine(parts)


def value(out) -> np.ndarray:
    """The pixels' values, out[..., 0] / out[..., 1]."""
    return bands.value(out)
