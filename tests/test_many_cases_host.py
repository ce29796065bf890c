"""The preconditions of test_gpu_many_exposures.py, checked with numpy alone: the sets of many_cases.py have the edges their
docstring promises, on the sides of 64 it promises them, and the references the device tests compare with -- xcor.sysrem_reference
at the (ncomp, niter) pairs used there, xcor.weighted_factor of its basis and of wfilter_cases.random_basis -- are finite and
leave most columns live.  A failure on the device is then no problem of the inputs."""
import numpy as np
import pytest

import many_cases as mc
import wfilter_cases as wc
from transit_amd import xcor

EXPOSURES = [("exp", n) for n in mc.NEXPS]
ORDERS = [("seg", n) for n in mc.NSEGS]


def the_set(kind, n):
    return mc.exposures_set(n) if kind == "exp" else mc.orders_set(n)


def ids(params):
    return ["%s%d" % p for p in params]


@pytest.mark.parametrize("nexp", mc.NEXPS)
def test_many_exposures_sets_have_their_edges(nexp):
    ms = mc.exposures_set(nexp)
    assert (ms.nexp, ms.nseg, ms.npix) == (nexp, 8, 800) and ms.lengths == [1, 63, 64, 65, 200, 0, 7, 400]
    assert sorted(ms.off_grid) == [250, 700]
    w = ms.weight
    assert w.shape == ms.data.shape == (nexp, 800) and np.isfinite(ms.data).all()
    assert w.min() == 0.0 and w[w > 0].min() >= 0.5 and w.max() <= 2.0
    assert 0.04 < np.count_nonzero(w == 0) / w.size < 0.07
    assert np.all(w[:, ms.masked_col] == 0) and np.all(w[ms.masked_exp, ms.segment(ms.masked_seg)] == 0)
    assert ms.masked_exp >= 64 or nexp == 64             # on the second trip of a wave over the exposures, where there is one
    others = np.delete(np.arange(nexp), ms.masked_exp)
    assert np.all(np.count_nonzero(w[others][:, ms.segment(ms.masked_seg)] > 0, axis=1) > 40)
    assert ms.gain.min() >= 0.5 and ms.gain.max() <= 1.5
    assert ms.velocity[0] == -40.0 and ms.velocity[-1] == 40.0 and np.all(np.diff(ms.shifts) < 0)
    # the table: scale 0 on both sides of 64 (where there is another side), smears with exact zeros among them
    zeros = np.flatnonzero(ms.scale == 0)
    assert zeros.min() < 64 and (zeros.max() >= 64 or nexp == 64) and zeros.size == {64: 3, 65: 4, 130: 5}[nexp]
    assert ms.scale.min() < 0 and 0.0 in ms.smear and ms.smear.max() > 1e-5 and ms.smear.max() <= 1.3e-5


@pytest.mark.parametrize("nseg", mc.NSEGS)
def test_many_orders_sets_have_their_edges(nseg):
    ms = mc.orders_set(nseg)
    assert (ms.nexp, ms.nseg) == (5, nseg) and ms.npix == sum(ms.lengths) <= 1500
    assert max(ms.lengths) == 64 and len(ms.off_grid) == 1
    empty = np.flatnonzero(np.array(ms.lengths) == 0)
    assert empty.min() < 64 and (nseg < 130 or empty.max() > 64)       # empty segments on both sides of 64
    dead = ms.dead_seg
    assert dead == min(64, nseg - 1) and ms.lengths[dead] == 5 and np.all(ms.weight[:, ms.segment(dead)] == 0)
    assert np.all(ms.weight[:, ms.masked_col] == 0) and np.all(ms.weight[ms.masked_exp, ms.segment(ms.masked_seg)] == 0)
    for p in list(ms.off_grid) + [ms.masked_col]:
        assert ms.seg_first[5] <= p < ms.seg_first[6]
    assert 3 in np.flatnonzero(ms.scale == 0)


@pytest.mark.parametrize("kind,n", EXPOSURES + ORDERS, ids=ids(EXPOSURES + ORDERS))
def test_every_live_row_has_pixels(kind, n):
    """every non-empty segment has a non-zero count at every exposure, the masked exposure of its segment and the dead segment
    apart -- the off-grid pixels, which count nowhere, left out"""
    ms = the_set(kind, n)
    on = np.ones(ms.npix, dtype=bool)
    on[list(ms.off_grid)] = False
    for s, length in enumerate(ms.lengths):
        count = np.count_nonzero((ms.weight[:, ms.segment(s)] > 0) & on[None, ms.segment(s)], axis=1)
        if length == 0 or s == ms.dead_seg:
            assert np.all(count == 0), s
        elif s == ms.masked_seg:
            assert count[ms.masked_exp] == 0 and np.all(np.delete(count, ms.masked_exp) > 0), s
        else:
            assert np.all(count > 0), s


@pytest.mark.parametrize("kind,n", EXPOSURES + ORDERS, ids=ids(EXPOSURES + ORDERS))
def test_one_cell_leaves_the_lag_grid_at_the_last_exposure_only(kind, n):
    ms = the_set(kind, n)
    for offset in (ms.offset, None):
        vm = ms.the_map(offset=offset)
        assert (vm.nkp, vm.nvsys) == (3, 4) and 9 <= vm.nlag <= 11
        idx = xcor.nearest_lags(vm)
        outside = idx < 0
        cells = np.argwhere(outside.any(axis=-1))
        assert cells.tolist() == [list(mc.OUTSIDE_CELL)]
        assert np.flatnonzero(outside[mc.OUTSIDE_CELL]).tolist() == [ms.nexp - 1]
        assert kind == "seg" or ms.nexp - 1 >= 63
        # the inside cells take lags from both ends of the grid
        assert idx[~outside].min() == 0 and idx[~outside].max() == vm.nlag - 1
        assert np.array_equal(np.isnan(xcor.map_from_per(np.ones((vm.nlag, ms.nexp)), vm)), outside.any(axis=-1))


def check_factor(ms, ob, basis, what):
    L, D, live = xcor.weighted_factor(ob, xcor.WeightedFilter(basis))
    assert np.count_nonzero(live) >= 0.75 * ms.npix, (what, np.count_nonzero(live))
    if ob.weight is not None:
        assert not live[ms.masked_col], what
        if ms.dead_seg is not None:
            assert not live[ms.segment(ms.dead_seg)].any(), what
    return int(np.count_nonzero(~live))


SYSREM = [("exp", n, c, i, w) for n in mc.NEXPS for (c, i) in mc.SYSREM_PAIRS for w in (False, True)] + [("seg", n, mc.ORDERS_NCOMP, 10, True) for n in mc.NSEGS]


@pytest.mark.parametrize("kind,n,ncomp,niter,weighted", SYSREM, ids=["%s%d-%d-%d-%s" % (k, n, c, i, "w" if w else "u") for k, n, c, i, w in SYSREM])
def test_the_sysrem_mirror_is_finite_and_its_filter_leaves_columns_live(kind, n, ncomp, niter, weighted):
    ms = the_set(kind, n)
    ob = ms.observed(weighted=weighted)
    basis, coef, resid = xcor.sysrem_reference(ob.data, ob.weight, ob.seg_first, ncomp, niter)
    assert basis.shape == (ms.nseg, ms.nexp, ncomp) and np.isfinite(basis).all() and np.isfinite(coef).all() and np.isfinite(resid).all()
    for s, length in enumerate(ms.lengths):
        if length == 0 or s == ms.dead_seg:
            assert np.all(basis[s] == 0), s
        else:
            assert np.any(basis[s, :, 0] != 0), s
    if weighted:
        assert np.all(basis[ms.masked_seg, ms.masked_exp] == 0) and not np.signbit(basis[ms.masked_seg, ms.masked_exp]).any()
    dead = check_factor(ms, ob, basis, (kind, n, ncomp, niter, weighted))
    print("%s, %d components of %d alternations, %s: %d of %d columns dead" % (ms.name, ncomp, niter, "weighted" if weighted else "no weights", dead, ms.npix))


RANDOM = [("exp", n, c) for n in mc.NEXPS for c in (4, 5, 8, 16)] + [("seg", n, mc.ORDERS_NCOMP) for n in mc.NSEGS]


@pytest.mark.parametrize("kind,n,ncomp", RANDOM, ids=["%s%d-%d" % p for p in RANDOM])
def test_a_random_basis_leaves_columns_live(kind, n, ncomp):
    ms = the_set(kind, n)
    dead = check_factor(ms, ms.observed(), wc.random_basis(ms.nseg, ms.nexp, ncomp, seed=50 + ncomp), (kind, n, ncomp))
    print("%s, a random basis of %d components: %d of %d columns dead" % (ms.name, ncomp, dead, ms.npix))
