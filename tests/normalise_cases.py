"""What the normalisation tests share (test_normalise_host.py, test_gpu_normalise.py): the recipe corners, and one set
beside sysrem_cases' at the selection kernel's edges -- a segment one pixel longer than the staging capacity (2048 keys, a
block's registers) and one exactly at it, rows of heavy ties (data rounded to integers), a row with all values equal,
negative values, a row fully masked and rows whose quantile is <= 0."""
import numpy as np

from transit_amd import xcor

CAP = 2048                                       # kNormCap of transit_amd/csrc/trx_normalise.h
LENGTHS = [CAP + 1, CAP, 33, 100]
SEG = xcor.segments(LENGTHS)
NPIX = int(SEG[-1])
OVER_SEG, AT_SEG, TIE_SEG, ODD_SEG = 0, 1, 2, 3
MASKED_SEG = AT_SEG                              # the last exposure is masked over the whole of this segment (with weights)
NEXPS = [1, 2, 7, 65]

ROWS = (xcor.NORM_ROW_NONE, xcor.NORM_ROW_QUANTILE)
COLS = (xcor.NORM_COL_NONE, xcor.NORM_COL_DIVIDE, xcor.NORM_COL_RATIO, xcor.NORM_COL_SUBTRACT)
QUANTILES = (0.0, 0.5, 0.9, 1.0)
CLIPS = (0.0, 3.0)


def recipes():
    """every recipe corner: each row kind times each column kind, quantile 0, 0.5, 0.9 and 1 (where the row kind reads it),
    clip 0 and 3 -- without the one recipe that does nothing, which trx_set_normalise refuses"""
    out = []
    for row in ROWS:
        for col in COLS:
            for q in (QUANTILES if row == xcor.NORM_ROW_QUANTILE else (0.5,)):
                for clip in CLIPS:
                    if row == xcor.NORM_ROW_NONE and col == xcor.NORM_COL_NONE and clip == 0:
                        continue
                    out.append(xcor.Normalise(row, col, q, clip))
    return out


def name(nm):
    return "row %d col %d q %g clip %g" % (nm.row_kind, nm.col_kind, nm.quantile, nm.clip)


def the_set(nexp: int, weighted: bool):
    """(data [nexp, NPIX], weights or None): a continuum of order 100 with a throughput per exposure and 1 % noise; exposure 0
    rounded to integers over the long segment (heavy ties); TIE_SEG small integers about 0 (ties, negative values, quantiles
    <= 0); ODD_SEG: exposure 0 all equal, exposure 1 all negative (a bad row at every quantile).  The weights mask 3 % single
    entries and the last exposure over MASKED_SEG."""
    rng = np.random.default_rng(900 + nexp)
    x, t = np.linspace(0.0, 1.0, NPIX), np.linspace(-1.0, 1.0, nexp) if nexp > 1 else np.zeros(1)
    cont = 100.0 * (1.0 + 0.3 * np.sin(9.0 * x))
    d = cont[None, :] * (1.0 + 0.2 * t[:, None]) * (1.0 + 0.01 * rng.standard_normal((nexp, NPIX)))
    a, b = int(SEG[OVER_SEG]), int(SEG[OVER_SEG + 1])
    d[0, a:b] = np.round(d[0, a:b] / 10.0)
    a, b = int(SEG[TIE_SEG]), int(SEG[TIE_SEG + 1])
    d[:, a:b] = np.round(2.0 * rng.standard_normal((nexp, b - a)))
    a, b = int(SEG[ODD_SEG]), int(SEG[ODD_SEG + 1])
    d[0, a:b] = 2.5
    if nexp > 1:
        d[1, a:b] = -np.abs(d[1, a:b])
    w = None
    if weighted:
        w = rng.uniform(0.5, 2.0, (nexp, NPIX))
        w[rng.random((nexp, NPIX)) < 0.03] = 0.0
        w[nexp - 1, SEG[MASKED_SEG]:SEG[MASKED_SEG + 1]] = 0.0
    return d, w

