"""The sets the SYSREM tests share (test_sysrem_host.py, test_gpu_sysrem.py): the segments of 800 pixels -- a tile of one
lane, 63, 64, 64 + 1, several tiles, an empty segment, 7, and more than one trip of the row kernel --, smooth trends plus
seeded noise, and the edge weights."""
import numpy as np

from transit_amd import xcor

LENGTHS = [1, 63, 64, 65, 200, 0, 7, 400]
SEG = xcor.segments(LENGTHS)
NPIX = int(SEG[-1])
MASKED_COL = 300                                 # masked at every exposure (in the 200-pixel segment)
MASKED_EXP, MASKED_SEG = 2, 3                    # exposure 2 masked over the whole 65-pixel segment


def data_set(nexp: int, seed: int, noise: float = 0.01, nterms: int = 6) -> np.ndarray:
    """[nexp, NPIX]: a continuum of order 1 times (1 + a few smooth trends in time of falling size) plus noise"""
    rng = np.random.default_rng(seed)
    x, t = np.linspace(0.0, 1.0, NPIX), np.linspace(-1.0, 1.0, nexp)
    cont = 1.0 + 0.3 * np.sin(7.0 * x) + 0.1 * np.cos(31.0 * x)
    d = np.ones((nexp, NPIX))
    for k in range(nterms):
        d += 0.2 * 0.4 ** k * rng.uniform(-1.0, 1.0, nexp)[:, None] * np.cos((3.0 + 5.0 * k) * x + rng.uniform(0, 6.0))[None, :] * (1.0 + 0.2 * t[:, None])
    return cont[None, :] * d * (1.0 + 0.05 * t[:, None]) + noise * rng.standard_normal((nexp, NPIX))


def edge_weights(nexp: int, seed: int) -> np.ndarray:
    """[nexp, NPIX]: weights in [0.5, 2) with 5 % single masked entries, MASKED_COL masked at every exposure and exposure
    MASKED_EXP masked over the whole of segment MASKED_SEG"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 2.0, (nexp, NPIX))
    w[rng.random((nexp, NPIX)) < 0.05] = 0.0
    w[:, MASKED_COL] = 0.0
    w[MASKED_EXP, SEG[MASKED_SEG]:SEG[MASKED_SEG + 1]] = 0.0
    return w

