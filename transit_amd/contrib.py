"""Contribution functions per wavenumber bin and layer from optical depths, in numpy (no GPU): the definition that
trx_run_contrib (include/transit_hip.h) reduces to bands on the device, for tests and for users without the device path.

Heights are counted as the optical-depth arrays count them (i = 0: the top layer; height i is atmosphere layer
nlayer-1-i; `last`: the ray's last height); every result is in the ATMOSPHERE's layer order (bottom first).

    from_tau(tau, last, temp, wn_cgs, angles_deg)   eclipse: F[bin, layer] = B W, the flux quadrature regrouped by node
    transmittance_from_tau(tau, last)               transit: exp(-tau) down to `last`, zero below
    planck(wn_cgs, temp)                            B[bin, layer]
    area_weights(angles_deg)                        the reference's area weights of the angles
    reduce(per_bin, band_bins, band_weights)        one band's row: sum_j w_j per_bin[j, :], correctly rounded
    combine(parts)                                  shard partial rows added in the order given (rank order)
    normalise(contrib)                              rows divided by their sum (a row of zeros stays zero)
    weighting(contrib, sums)                        transit: differences of the band-averaged transmittance
"""
from __future__ import annotations

import math

import numpy as np

# physical constants of the reference (cgs), as the kernels carry them
H, LS, KB = 6.6260755e-27, 2.99792458e10, 1.380658e-16


def planck(wn_cgs, temp) -> np.ndarray:
    """B[bin, layer] = 2 h w^3 c^2 / (exp(h w c / (k T)) - 1), w in cm-1 (the grid times wn_fct)."""
    w = np.asarray(wn_cgs, dtype=np.float64)[:, None]
    t = np.asarray(temp, dtype=np.float64)[None, :]
    return (2.0 * H * w ** 3 * LS * LS) / (np.exp(H * w * LS / (KB * t)) - 1.0)


def area_weights(angles_deg) -> np.ndarray:
    """sin^2(grid[a+1]) - sin^2(grid[a]), grid = 0, the midpoints of neighbouring angles, 90 degrees."""
    a = np.asarray(angles_deg, dtype=np.float64)
    deg = math.pi / 180.0
    grid = np.zeros(a.size + 1)
    grid[a.size] = 90.0 * deg
    grid[1:a.size] = (a[:-1] + a[1:]) * deg / 2.0
    return np.sin(grid[1:]) ** 2 - np.sin(grid[:-1]) ** 2


def _heights(tau, last):
    tau = np.asarray(tau, dtype=np.float64)
    last = np.asarray(last).astype(np.int64)
    if tau.ndim != 2 or last.shape != (tau.shape[0],):
        raise ValueError("tau: [bins, heights] (top first), last: [bins]")
    i = np.arange(tau.shape[1])[None, :]
    have = i <= last[:, None]
    return np.where(have, tau, 0.0), last, i, have      # (entries below `last` are not defined: never used)


def from_tau(tau, last, temp, wn_cgs, angles_deg) -> np.ndarray:
    """Eclipse geometry.  tau [bins, heights] (height 0 = top), last [bins], temp [layers] (atmosphere order),
    wn_cgs [bins], angles in degrees.  Returns F [bins, layers], atmosphere order:

        g_i = pi sum_a area_a exp(-tau_i / cos a),  d_i = g_i - g_{i+1}
        W_0 = d_0 / 2,  W_i = (d_{i-1} + d_i) / 2,  W_last = d_{last-1} / 2 + g_last,  W_i = 0 below last
        F_i = B_i W_i     (sum_i F_i: the flux of the bin; every term >= 0)
    """
    tau, last, i, have = _heights(tau, last)
    ang = np.asarray(angles_deg, dtype=np.float64) * (math.pi / 180.0)
    area = area_weights(angles_deg)
    g = np.zeros_like(tau)
    for a in range(ang.size):
        g = g + area[a] * np.exp(-tau / math.cos(ang[a]))
    g = np.where(have, math.pi * g, 0.0)
    d = np.zeros_like(g)
    d[:, :-1] = g[:, :-1] - g[:, 1:]
    d = np.where(i < last[:, None], d, 0.0)
    W = 0.5 * d
    W[:, 1:] = 0.5 * (d[:, :-1] + d[:, 1:])
    W = W + np.where(i == last[:, None], g, 0.0)
    B = planck(wn_cgs, temp)[:, ::-1]                   # height order
    return (B * W)[:, ::-1].copy()


def transmittance_from_tau(tau, last) -> np.ndarray:
    """Transit geometry: T [bins, layers] (atmosphere order) = exp(-tau_i) for i <= last, 0 below."""
    tau, last, i, have = _heights(tau, last)
    return np.where(have, np.exp(-tau), 0.0)[:, ::-1].copy()


def reduce(per_bin, band_bins, band_weights) -> np.ndarray:
    """One band's row [layers]: sum over the band's bins j of w_j per_bin[j, :], each sum correctly rounded
    (math.fsum).  band_bins index per_bin's first axis (a shard: the bins local to it)."""
    per_bin = np.asarray(per_bin, dtype=np.float64)
    bins = np.asarray(band_bins, dtype=np.int64)
    w = np.asarray(band_weights, dtype=np.float64)
    if bins.shape != w.shape:
        raise ValueError("reduce: one weight per bin")
    terms = w[:, None] * per_bin[bins, :]
    return np.array([math.fsum(terms[:, r]) for r in range(per_bin.shape[1])])


def combine(parts) -> np.ndarray:
    """Partial rows of the shards ([nbands][nlayer] each), added in the order given -- rank order for the job's."""
    parts = [np.asarray(p, dtype=np.float64) for p in parts]
    if not parts:
        raise ValueError("combine: no partial rows")
    out = parts[0].copy()
    for p in parts[1:]:
        out = out + p
    return out


def normalise(contrib) -> np.ndarray:
    """Rows divided by their sum; a row that sums to zero stays zero."""
    c = np.asarray(contrib, dtype=np.float64)
    s = c.sum(axis=-1, keepdims=True)
    out = np.zeros_like(c)
    np.divide(c, s, out=out, where=s != 0)
    return out


def weighting(contrib, sums) -> np.ndarray:
    """Transit geometry: the band-averaged transmittance contrib[b] / sums[b][1] differenced between neighbouring
    layers, [nbands, nlayer-1] (entry r: layer r+1 minus layer r).  A band of zero weight gives zeros."""
    c = np.asarray(contrib, dtype=np.float64)
    sw = np.asarray(sums, dtype=np.float64)[..., 1][..., None]
    t = np.zeros_like(c)
    np.divide(c, sw, out=t, where=sw != 0)
    return t[..., 1:] - t[..., :-1]
