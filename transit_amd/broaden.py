"""Host side of the rotational broadening, Engine.set_broadening / Engine.run_broadened and their Batch forms
(trx_set_broadening / trx_run_broadened, include/transit_hip.h).

A broadening is the planet's rotation kernel (Gray's profile with linear limb darkening) applied to the spectrum on the
device before the detector pixels sample it.  On the grid nu_i = wn_i + i wn_d bin i gets a window of h_i =
floor(nu_i beta / wn_d) bins on either side, beta = v sin i / c:

    Rotation(v_kms, limb=0.6)                a broadening; Rotation.from_beta(beta, limb) takes beta as it is
    half_widths(wn_i, wn_d, nwn, beta)       the integers h_i, computed in double as the device computes them
    reference(spec, wn_i, wn_d, b)           the definition: weights in np.longdouble from the double x, sums by math.fsum
    bound(spec, wn_i, wn_d, b)               the per-bin tolerance of a double-precision evaluation against reference

An extra GAUSSIAN velocity broadening needs none of this: add its FWHM to the pixels' fwhm in quadrature.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np

from . import _abi
from .pixels import C_KMS

MAX_HALF = _abi.BROADEN_MAX_HALF
EPS = 2.0 ** -52


@dataclass
class Rotation:
    """One trx_broadening of kind ROTATION: v sin i in km/s (beta = v_kms / C_KMS) and the limb-darkening
    coefficient in [0, 1]."""
    v_kms: float
    limb: float = 0.6
    beta: float = field(init=False)

    def __post_init__(self):
        self.v_kms, self.limb = float(self.v_kms), float(self.limb)
        self.beta = self.v_kms / C_KMS

    @classmethod
    def from_beta(cls, beta: float, limb: float = 0.6) -> "Rotation":
        b = cls(float(beta) * C_KMS, limb)
        b.beta = float(beta)
        return b


def to_c(b: Rotation) -> _abi.TrxBroadening:
    return _abi.TrxBroadening(_abi.BROADEN_ROTATION, 0, b.beta, b.limb)


def _halves(wn_i: float, wn_d: float, nwn: int, beta: float):
    """(h_i as int64, d_i): every operation a numpy double operation of its own, rounded once."""
    nu = float(wn_i) + np.arange(int(nwn), dtype=np.float64) * float(wn_d)
    d = nu * float(beta)
    return np.floor(d / float(wn_d)).astype(np.int64), d


def half_widths(wn_i: float, wn_d: float, nwn: int, beta: float) -> np.ndarray:
    """h_i = floor((wn_i + i wn_d) beta / wn_d) for i < nwn, in double; non-decreasing."""
    return _halves(wn_i, wn_d, nwn, beta)[0]


def weights(limb: float):
    """(c1, c2) of w(x) = c1 sqrt(1 - x^2) + c2 (1 - x^2), in double."""
    return 2.0 * (1.0 - float(limb)), (math.pi / 2.0) * float(limb)


def _split_sums(rows) -> np.ndarray:
    """math.fsum along the rows of longdouble terms: each term as its double and what the double left over."""
    hi = rows.astype(np.float64)
    lo = (rows - hi).astype(np.float64)
    return np.array([math.fsum(r) for r in np.concatenate([hi, lo], axis=1).tolist()])


def _windows(spec, wn_i, wn_d, b: Rotation, bins, chunk=256):
    """Per chunk of output bins I with h > 0: (I, t, w, S_below, S_above, in_below, in_above) -- t the double-x
    (1 - x^2 clipped at 0) and w the weights, both longdouble [len(I), H], zero beyond a bin's own h."""
    n = spec.size
    h, d = _halves(wn_i, wn_d, n, b.beta)
    c1, c2 = weights(b.limb)
    bins = np.arange(n) if bins is None else np.asarray(bins, dtype=np.int64).reshape(-1)
    live = bins[h[bins] > 0]
    L = np.longdouble
    for a in range(0, live.size, chunk):
        I = live[a:a + chunk]
        H = int(h[I].max())
        k = np.arange(1, H + 1)
        x = (k.astype(np.float64)[None, :] * float(wn_d)) / d[I][:, None]
        mine = k[None, :] <= h[I][:, None]
        xl = x.astype(L)
        t = np.maximum(L(0), L(1) - xl * xl)
        w = np.where(mine, L(c1) * np.sqrt(t) + L(c2) * t, L(0))
        lo, hi = I[:, None] - k[None, :], I[:, None] + k[None, :]
        in_lo, in_hi = mine & (lo >= 0), mine & (hi < n)
        s_lo = np.where(in_lo, spec[np.clip(lo, 0, n - 1)], 0.0)
        s_hi = np.where(in_hi, spec[np.clip(hi, 0, n - 1)], 0.0)
        yield I, t, w, s_lo, s_hi, in_lo, in_hi


@functools.lru_cache(maxsize=8)
def _denominators(wn_i: float, wn_d: float, n: int, beta: float, limb: float) -> np.ndarray:
    """The sum of the weights actually used, per bin of the whole grid (1 where h = 0): it does not depend on the
    spectrum, so the references of several spectra under one broadening share it."""
    L = np.longdouble
    c1, c2 = weights(limb)
    den = np.ones(n)
    for I, _, w, _, _, in_lo, in_hi in _windows(np.zeros(n), wn_i, wn_d, Rotation.from_beta(beta, limb), None):
        den[I] = _split_sums(np.concatenate([np.full((I.size, 1), L(c1) + L(c2)), w * in_lo, w * in_hi], axis=1))
    den.setflags(write=False)
    return den


def reference(spec, wn_i: float, wn_d: float, b: Rotation, bins=None) -> np.ndarray:
    """The definition over the whole-grid spectrum `spec`: B_i for every bin (or for `bins`, in that order).  x as the
    definition's double, the weights and products in np.longdouble, numerator and denominator by math.fsum (each
    rounded to double once; their quotient in long double: B_i is within 1.5 ulp of the exact value)."""
    spec = np.ascontiguousarray(spec, dtype=np.float64).reshape(-1)
    L = np.longdouble
    c1, c2 = weights(b.limb)
    w0 = L(c1) + L(c2)
    out = spec.copy()                                   # (h = 0: a copy)
    den_all = _denominators(float(wn_i), float(wn_d), spec.size, b.beta, b.limb) if bins is None else None
    for I, _, w, s_lo, s_hi, in_lo, in_hi in _windows(spec, wn_i, wn_d, b, bins):
        centre = np.full((I.size, 1), w0)
        num = _split_sums(np.concatenate([centre * spec[I][:, None].astype(L), w * s_lo, w * s_hi], axis=1))
        den = den_all[I] if den_all is not None else _split_sums(np.concatenate([centre, w * in_lo, w * in_hi], axis=1))
        out[I] = (num.astype(L) / den.astype(L)).astype(np.float64)
    return out if bins is None else out[np.asarray(bins, dtype=np.int64).reshape(-1)]


def bound(spec, wn_i: float, wn_d: float, b: Rotation, bins=None, ref=None) -> np.ndarray:
    """tol_i = A_i (2 h_i + 17) 2^-52 + E_i per bin (or per entry of `bins`; ref: reference() of the same arguments,
    when the caller has it already):
    A_i = sum of w |S| / sum of w covers the summation in double and the final division;
    E_i = sum over the window's bins of c1 min(sqrt(e), e / sqrt(t)) |S - B_i| / sum of w, e = 8 * 2^-52, bounds what a
    few ulps in 1 - x^2 do to the square root near the profile's edge (where its slope is unbounded)."""
    spec = np.ascontiguousarray(spec, dtype=np.float64).reshape(-1)
    n = spec.size
    h = half_widths(wn_i, wn_d, n, b.beta)
    c1, c2 = weights(b.limb)
    w0 = c1 + c2
    B = spec.copy()
    B[np.arange(n) if bins is None else np.asarray(bins, dtype=np.int64).reshape(-1)] = reference(spec, wn_i, wn_d, b, bins) if ref is None else ref
    tol = np.abs(spec) * 17.0 * EPS                     # (h = 0)
    e = 8.0 * EPS
    for I, t, w, s_lo, s_hi, in_lo, in_hi in _windows(spec, wn_i, wn_d, b, bins):
        t, w = t.astype(np.float64), w.astype(np.float64)
        den = w0 + np.sum(w * in_lo, axis=1) + np.sum(w * in_hi, axis=1)
        A = (w0 * np.abs(spec[I]) + np.sum(w * np.abs(s_lo), axis=1) + np.sum(w * np.abs(s_hi), axis=1)) / den
        with np.errstate(divide="ignore"):
            slope = c1 * np.minimum(math.sqrt(e), e / np.sqrt(t))
        dev = np.where(in_lo, np.abs(s_lo - B[I][:, None]), 0.0) + np.where(in_hi, np.abs(s_hi - B[I][:, None]), 0.0)
        E = np.sum(slope * dev, axis=1) / den
        tol[I] = A * (2.0 * h[I] + 17.0) * EPS + E
    return tol if bins is None else tol[np.asarray(bins, dtype=np.int64).reshape(-1)]
