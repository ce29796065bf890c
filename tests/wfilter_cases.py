"""Inputs shared by the weighted filter's tests (tests/test_wfilter_host.py, tests/test_gpu_wfilter.py): the bases, the
weights with their edge columns, and the precondition that no live/dead decision hinges on a pivot's last bits."""
import numpy as np

from transit_amd import _abi, xcor


def random_basis(nseg, nexp, ncomp, seed):
    """[nseg, nexp, ncomp]: per segment ncomp random unit vectors, the first min(ncomp, nexp) of them orthonormal (the Q
    of a QR) -- with ncomp > nexp the vectors beyond nexp depend on the others, and every column of the set is singular"""
    rng = np.random.default_rng(seed)
    out = np.zeros((nseg, nexp, ncomp))
    for s in range(nseg):
        a = rng.standard_normal((nexp, ncomp))
        a[:, :nexp] = np.linalg.qr(a[:, :nexp])[0]
        out[s] = a / np.linalg.norm(a, axis=0)
    return out


def edge_weights(nexp, npix, ncomp, masked, short, exact, seed, scattered=0.1):
    """[nexp, npix] weights in [0.5, 2]; the share `scattered` of the columns, otherwise ordinary, has ONE masked entry each;
    column `masked` is 0 at every exposure; column `short` has exactly ncomp - 1 positive weights (none for
    ncomp - 1 > nexp: the column is then masked whole); column `exact` exactly min(ncomp, nexp) positive weights"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 2.0, (nexp, npix))
    cols = np.flatnonzero(rng.random(npix) < scattered)
    w[rng.integers(0, nexp, cols.size), cols] = 0.0
    w[:, masked] = 0.0
    for col, keep in ((short, ncomp - 1), (exact, ncomp)):
        w[:, col] = rng.uniform(0.5, 2.0, nexp)
        keep = min(keep, nexp) if col == exact else (keep if keep <= nexp else 0)
        w[rng.permutation(nexp)[keep:], col] = 0.0
        assert np.count_nonzero(w[:, col] > 0) == keep
    return w


def decisive(obs, wf, lo=2.0 ** -40, hi=2.0 ** -12):
    """The precondition: walking every column's pivots in order up to its first singular one, each pivot's share
    D_j / N_jj of its diagonal entry is above `hi` (good) or it is below `lo` -- N_jj = 0 included -- (singular).  What
    follows a singular pivot decides nothing.  Returns the live flags, asserted to be weighted_factor's."""
    assert lo < _abi.WFILTER_PIVOT < hi
    ratio = xcor.weighted_pivots(obs, wf)
    L, D, live = xcor.weighted_factor(obs, wf)
    alive = np.ones(obs.npix, dtype=bool)
    for j in range(wf.ncomp):
        r = ratio[:, j]
        good = r > hi
        with np.errstate(invalid="ignore"):
            bad = ~(r >= lo)                             # below lo, or nan: N_jj = 0
        assert np.all(good[alive] | bad[alive]), (j, r[alive & ~good & ~bad])
        alive = alive & good
    assert np.array_equal(alive, live)
    return live
