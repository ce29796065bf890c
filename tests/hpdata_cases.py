"""What the tests of the observed set's own high-pass share (test_hpdata_host.py, test_gpu_hpdata.py): scatter_cases' sets
over two segmentations of the same 800 pixels, raw and after the numpy SYSREM, the halves and the tables, and the numpy
composition the mirror is held against.

  SEGS["orders"]   scatter_cases' segments: 1, 63, 64, 65, 200, 0, 7 and 400 pixels -- every tile is a segment's only one
  SEGS["long"]     1, 63, 0 and 736 pixels: the last segment spans two tiles of kHpTile = 512, the second ragged (224), with
                   the tile border at pixel BORDER = 64 + 512
"""
import numpy as np

import scatter_cases as cs
from transit_amd import xcor

TILE = 512                                             # kHpTile
SEGS = {"orders": cs.SEG, "long": xcor.segments([1, 63, 0, 736])}
BORDER = 64 + TILE
HALVES = (0, 1, 5, 70, 450)
NEAR = 5                                               # a masked entry this close to BORDER on either side, in every weighted set
STAGES = ("raw", "detrended")


def tables(half, seed=0):
    """a boxcar, a Gaussian and a random table (a fifth of its taps zero) of this half: test_gpu_highpass.tables"""
    rng = np.random.default_rng(1000 + half + seed)
    rnd = np.concatenate([[0.7], rng.uniform(0.0, 2.0, half) * (rng.random(half) > 0.2)])
    gauss = np.exp(-(np.arange(half + 1.0) ** 2) / (2.0 * max(half / 3.0, 0.5) ** 2))
    return {"boxcar": xcor.boxcar_highpass(2 * half + 1), "gauss": xcor.HighPass(gauss), "random": xcor.HighPass(rnd)}


_DATA = {}


def the_data(nexp, weighted, stage, seg_name, scale=1.0):
    """(data [nexp, 800] the high-pass reads, weight or None): scatter_cases.the_set, raw or its residuals after
    xcor.sysrem_reference(.., 3, 2) over the segmentation -- made once and left unchanged"""
    key = (nexp, weighted, stage, seg_name, scale)
    if key not in _DATA:
        d, w, _ = cs.the_set(nexp, weighted, scale)
        if stage == "detrended":
            d = xcor.sysrem_reference(d, w, SEGS[seg_name], 3, 2)[2]
            d.setflags(write=False)
        _DATA[key] = (d, w)
    return _DATA[key]


def composition(d, w, seg, hp):
    """the definition through the model's own reference: highpass_reference of the pairs (d, W > 0) without a gain, NaN -> +0"""
    live = np.ones(d.shape) if w is None else (w > 0).astype(np.float64)
    v = xcor.highpass_reference(np.stack([d, live], -1), xcor.Observed(seg, d, None, None), hp)
    return np.where(np.isnan(v), 0.0, v)


def alone(w, seg, hp, shape):
    """[nexp, npix] bool: the live entries with no OTHER live entry of their segment under a non-zero tap of their window --
    their running mean is their own value"""
    live = np.ones(shape, dtype=bool) if w is None else w > 0
    others = np.zeros(shape)
    for s in range(len(seg) - 1):
        a, b = int(seg[s]), int(seg[s + 1])
        for k in range(1, hp.half + 1):
            if hp.taps[k] > 0 and k < b - a:
                others[:, a:b - k] += live[:, a + k:b]
                others[:, a + k:b] += live[:, a:b - k]
    return live & (others == 0)
