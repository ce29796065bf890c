"""The sets the column-scatter tests share (test_scatter_host.py, test_gpu_scatter.py): sysrem_cases' segments of 800 pixels
-- 1, 63, 64, 65, 200, 0, 7 and 400 --, a continuum with faint smooth trends in time plus seeded noise, sysrem_cases'
edge weights, and the planted columns:

  CONSTANT_COL   a constant column of the 63-pixel segment: var = 0, dead
  MASKED_COL     sysrem_cases': masked at every exposure under the edge weights: n = 0, dead
  NOISY_COLS     five columns of the 400-pixel segment with 10 x the noise: the ones a clip of 3 removes
  the ties       in the 65-pixel and in the 200-pixel segment the column of the median rank (m - 1) // 2 is copied, data and
                 weights, onto the column of the next rank: two identical columns straddle the median, for an odd and an even
                 number of live columns (without weights: m = 65 and m = 200)
"""
import numpy as np

import sysrem_cases as sc
from transit_amd import xcor

SEG, NPIX, LENGTHS = sc.SEG, sc.NPIX, sc.LENGTHS
MASKED_COL = sc.MASKED_COL
CONSTANT_COL = 10
NOISY_COLS = (437, 500, 611, 700, 790)
TIE_SEGS = (3, 4)                                # the 65-pixel and the 200-pixel segment
NOISE = 0.01

KINDS = (xcor.SCATTER_VARIANCE, xcor.SCATTER_MASK)
CLIPS = (0.0, 3.0)


def ranked(var, s):
    """the live columns of segment s in the order of the definition: ascending var, ties by ascending pixel"""
    a, b = int(SEG[s]), int(SEG[s + 1])
    live = np.flatnonzero(var[a:b] > 0)
    return a + live[np.argsort(var[a:b][live], kind="stable")]


def plant_ties(data, weight):
    """(pairs): per TIE_SEGS segment the median column's data and weights copied onto the next column in rank; returns the
    (median column, its copy) pairs"""
    var = xcor.scatter_reference(data, weight, SEG, xcor.SCATTER_MASK)[0]
    pairs = []
    for s in TIE_SEGS:
        order = ranked(var, s)
        a, b = int(order[(order.size - 1) // 2]), int(order[(order.size - 1) // 2 + 1])
        data[:, b] = data[:, a]
        if weight is not None:
            weight[:, b] = weight[:, a]
        pairs.append((a, b))
    return pairs


_SETS = {}


def the_set(nexp: int, weighted: bool, scale: float = 1.0):
    """(data [nexp, NPIX], weight or None, tie pairs), made once per (nexp, weighted, scale)"""
    key = (nexp, weighted, scale)
    if key not in _SETS:
        rng = np.random.default_rng(300 + nexp)
        x, t = np.linspace(0.0, 1.0, NPIX), np.linspace(-1.0, 1.0, nexp)
        cont = 1.0 + 0.3 * np.sin(7.0 * x) + 0.1 * np.cos(31.0 * x)
        d = cont[None, :] * (1.0 + 2e-3 * t[:, None] * np.cos(5.0 * x)[None, :]) + NOISE * rng.standard_normal((nexp, NPIX))
        for p in NOISY_COLS:
            d[:, p] = cont[p] + 10.0 * NOISE * rng.standard_normal(nexp)
        d[:, CONSTANT_COL] = 1.25
        d *= scale
        w = sc.edge_weights(nexp, 50 + nexp) if weighted else None
        ties = plant_ties(d, w)
        d.setflags(write=False)
        if w is not None:
            w.setflags(write=False)
        _SETS[key] = (d, w, ties)
    return _SETS[key]


def clip_margin(var, med, keep, seg=SEG):
    """(clipped columns, the smallest | var / (9 med) - 1 | over the live columns): how far the clip of 3 is from flipping"""
    medp = np.repeat(med, np.diff(seg))
    live = var > 0
    ratio = var[live] / medp[live]
    return tuple(int(p) for p in np.flatnonzero(live & ~keep)), float(np.min(np.abs(ratio / 9.0 - 1.0)))
