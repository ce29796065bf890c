"""Host-side builders of instrument bands for Engine.set_bands / Batch.set_bands (trx_set_bands,
include/transit_hip.h).

A band is a weight per coarse bin of the whole wavenumber grid; a band run returns, per band, the pair
(sum of w_i S_i, sum of w_i) over the bins of the handle's shard, and the band's value is their ratio:

    tophat(wn, lo, hi)                    the box [lo, hi]: each bin weighted by the part of its cell inside it
    filter_curve(wn, filter_wn, trans)    a filter's transmission curve (BART's band integral)
    gauss(centre, fwhm, cut=4)            a Gaussian line-spread function, evaluated on the device
    resolving_power(centres, R, cut=4)    Gaussians of fwhm = centre / R at pixel centres
    combine(parts)                        shard partial sums added in the order given (rank order)
    value(sums)                           sums[..., 0] / sums[..., 1]
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _abi

FWHM_PER_SIGMA = 2.0 * math.sqrt(2.0 * math.log(2.0))


@dataclass
class Band:
    """One trx_band: kind WEIGHTS (weights of bins first .. first+len(weights)-1) or GAUSS."""
    kind: int
    first: int = 0
    weights: Optional[np.ndarray] = None
    centre: float = 0.0
    fwhm: float = 0.0
    cut: float = 0.0


def weights(first: int, w) -> Band:
    """A band of explicit weights for bins first, first+1, ... of the whole grid."""
    return Band(_abi.BAND_WEIGHTS, int(first), np.ascontiguousarray(w, dtype=np.float64))


def _spacing(wn) -> float:
    wn = np.asarray(wn, dtype=np.float64)
    if wn.ndim != 1 or wn.size < 2:
        raise ValueError("wn: the grid's wavenumbers, at least two")
    return float(wn[1] - wn[0])


def tophat(wn, lo: float, hi: float) -> Band:
    """Weight of bin i = the length of its cell [wn_i - d/2, wn_i + d/2] inside [lo, hi], divided by d
    (d: the grid spacing); the band holds the bins with a positive weight."""
    wn = np.asarray(wn, dtype=np.float64)
    d = _spacing(wn)
    if not hi > lo:
        raise ValueError("tophat: hi must exceed lo")
    w = (np.minimum(wn + d / 2, hi) - np.maximum(wn - d / 2, lo)) / d
    w = np.clip(w, 0.0, 1.0)
    nz = np.flatnonzero(w > 0)
    if nz.size == 0:
        raise ValueError("tophat: [%g, %g] covers no bin of the grid" % (lo, hi))
    return weights(nz[0], w[nz[0]:nz[-1] + 1])


def trapezoid_weights(x) -> np.ndarray:
    """c_i with sum(c_i y_i) = np.trapezoid(y, x)."""
    x = np.asarray(x, dtype=np.float64)
    c = np.zeros(x.size)
    dx = np.diff(x)
    c[:-1] += dx / 2
    c[1:] += dx / 2
    return c


def filter_curve(wn, filter_wn, transmission) -> Band:
    """BART's band integral: the transmission, linearly interpolated onto the grid points inside the filter's
    span, times the trapezoid weights of those points -- so that the band's value is
    np.trapezoid(f * S, x) / np.trapezoid(f, x) on those points x."""
    wn = np.asarray(wn, dtype=np.float64)
    fw = np.asarray(filter_wn, dtype=np.float64)
    ft = np.asarray(transmission, dtype=np.float64)
    if fw.shape != ft.shape or fw.size < 2:
        raise ValueError("filter_curve: wavenumbers and transmission of the same length, at least two")
    order = np.argsort(fw)
    fw, ft = fw[order], ft[order]
    idx = np.flatnonzero((wn >= fw[0]) & (wn <= fw[-1]))
    if idx.size < 2:
        raise ValueError("filter_curve: the filter covers fewer than two grid points")
    x = wn[idx[0]:idx[-1] + 1]
    f = np.interp(x, fw, ft)
    return weights(idx[0], f * trapezoid_weights(x))


def gauss(centre: float, fwhm: float, cut: float = 4.0) -> Band:
    """A Gaussian line-spread function: w_i = exp(-((nu_i - centre)/sigma)^2 / 2), sigma = fwhm / (2 sqrt(2 ln 2)),
    over the bins within cut sigmas of the centre (gauss_range)."""
    return Band(_abi.BAND_GAUSS, centre=float(centre), fwhm=float(fwhm), cut=float(cut))


def resolving_power(centres, R: float, cut: float = 4.0):
    """Gaussians at the given pixel centres, fwhm = centre / R."""
    return [gauss(c, float(c) / R, cut) for c in np.asarray(centres, dtype=np.float64)]


def gauss_range(wn_i: float, wn_d: float, nwn: int, centre: float, fwhm: float, cut: float):
    """The bins [i_lo, i_hi) of a GAUSS band, by the rule of trx_set_bands (in double, clipped to [0, nwn))."""
    sigma = fwhm / FWHM_PER_SIGMA
    a = math.ceil((centre - cut * sigma - wn_i) / wn_d)
    z = math.floor((centre + cut * sigma - wn_i) / wn_d) + 1
    a, z = min(max(a, 0), nwn), min(max(z, 0), nwn)
    return a, max(a, z)


def to_c(bands: Sequence[Band]):
    """The trx_band array of a set (the weights arrays stay owned by the Band objects)."""
    arr = (_abi.TrxBand * max(len(bands), 1))()
    for k, b in enumerate(bands):
        c = arr[k]
        c.kind = int(b.kind)
        if b.weights is not None:
            w = np.ascontiguousarray(b.weights, dtype=np.float64)
            b.weights = w
            c.first, c.n, c.weights = int(b.first), int(w.size), w.ctypes.data_as(_abi.c_double_p)
        else:
            c.first, c.n = int(b.first), 0
        c.centre, c.fwhm, c.cut = float(b.centre), float(b.fwhm), float(b.cut)
    return arr


def combine(parts) -> np.ndarray:
    """Partial sums of the shards ([nbands][2] each), added in the order given -- rank order for the
    job's sums."""
    parts = [np.asarray(p, dtype=np.float64) for p in parts]
    if not parts:
        raise ValueError("combine: no partial sums")
    out = parts[0].copy()
    for p in parts[1:]:
        out = out + p
    return out


def value(sums) -> np.ndarray:
    """The bands' values, sums[..., 0] / sums[..., 1]."""
    s = np.asarray(sums, dtype=np.float64)
    return s[..., 0] / s[..., 1]
