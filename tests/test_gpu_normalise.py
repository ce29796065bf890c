"""Normalising the observed set on the device, ahead of SYSREM and PCA (trx_set_normalise, trx_normalise_observed and step
1b of trx_detrend_observed and trx_pca_observed, include/transit_hip.h), against xcor.normalise_reference -- the numpy
mirror, whose quantile comes from a full sort -- BIT FOR BIT: data, row scales, centres and the two counts at every recipe
corner over sysrem_cases' sets (segments of 1, 63, 64, 65, 200, 0, 7 and 400 pixels, the edge weights) and
normalise_cases' set (a segment one pixel above the selection kernel's staging capacity and one at it, heavy ties, an
all-equal row, negative values, a masked row, rows whose quantile is <= 0) at 1, 2, 7 and 65 exposures; the detrending calls
with a recipe installed against sysrem_reference and pca_reference of the mirror's data, with and without injection; the
state the three calls share; and the refusals by code and message.

The problem is observed_cases.build_case's: pixel_cases.make("eclipse", 20 000 lines, 6001 bins) and its 800 pixels.  The refusals of
trx_normalise_observed's injection arguments are trx_detrend_observed's own code path (detrend_inject_checks), and its
refusal of a shard cannot be reached on a device -- no recipe can be installed on a shard, and "no recipe" is checked
first --: tests/normalise_check.cpp holds their text and their order on the host."""
import ctypes as C

import numpy as np
import pytest

import normalise_cases as nc
import observed_cases as oc
import pixel_cases as pc
import sysrem_cases as sc
from bits import same_bits
from transit_amd import _abi, pixels, xcor
from transit_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

SHIFTS = pc.SHIFTS
Q, NONE = xcor.NORM_ROW_QUANTILE, xcor.NORM_ROW_NONE
DIVIDE, SUBTRACT = xcor.NORM_COL_DIVIDE, xcor.NORM_COL_SUBTRACT


class Case(oc.SysremCase):
    def __init__(self, *a):
        super().__init__(*a)
        self.edge_px = pixels.resolving_power(np.linspace(2503.0, 2557.0, nc.NPIX), 20000.0, 4.0)

    def make_observed(self, nexp, weighted):
        """the SYSREM tests' raw set, with edge weights down to one exposure"""
        w = sc.edge_weights(max(nexp, 3), 80 + nexp)[:nexp].copy() if weighted else None
        return xcor.Observed(sc.SEG, self.scale * sc.data_set(nexp, 70 + nexp), w, self.gain(nexp))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return oc.build_case(tmp_path_factory.mktemp("normalise"), Case)


# ---- 1. every recipe corner, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("nexp", nc.NEXPS)
@pytest.mark.parametrize("which", ["sysrem set, edge weights", "sysrem set, no weights", "edge set, weights"])
def test_every_recipe_corner_is_the_mirrors_bit_for_bit(case, which, nexp):
    if which.startswith("sysrem"):
        ob, px = case.observed(nexp, "no weights" not in which), None
    else:
        data, w = nc.the_set(nexp, True)
        ob, px = xcor.Observed(nc.SEG, data, w), case.edge_px
    E = case.handle(ob, px)
    clipped = bad = 0
    for nm in nc.recipes():
        what = "%s, nexp %d, %s" % (which, nexp, nc.name(nm))
        E.set_normalise(nm)
        N = E.normalise_observed()
        mirror = xcor.normalise_reference(ob.data, ob.weight, ob.seg_first, nm)
        oc.check_normalised(N, mirror, what)
        assert N.spectrum is None and np.isfinite(N.data).all() and not np.signbit(N.rowscale).any(), what
        clipped, bad = clipped + N.nclipped, bad + N.nbad
    if which.startswith("edge"):
        # the edges took part: bad rows (a quantile <= 0) at every exposure count, the masked row, the all-equal row
        scale = xcor.normalise_reference(ob.data, ob.weight, ob.seg_first, oc.MEDIAN_RATIO)[1]
        assert bad > 0 and scale[nexp - 1, nc.MASKED_SEG] == 0 and scale[0, nc.ODD_SEG] == 2.5 and np.all(scale[:, nc.OVER_SEG] > 0)
    if nexp == 65:
        assert clipped > 0, which                            # (a clip of 3 sigma takes entries of 65)
    print("%s, nexp %d: %d recipes in the mirror's bits; %d entries clipped, %d bad over all of them" % (which, nexp, len(nc.recipes()), clipped, bad))
    E.close()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nexp", [8, 9, 16, 17])
def test_bits_about_a_whole_number_of_trips(case, nexp, weighted):
    """the column kernel takes 8 exposures a trip (kSysTrips): one and two whole trips, and one exposure past each; a recipe
    with a row quantile, a column mean and a clip takes every pass of it"""
    nm = xcor.Normalise(Q, DIVIDE, 0.9, 3.0)
    ob = case.observed(nexp, weighted)
    E = case.handle(ob)
    E.set_normalise(nm)
    mirror = xcor.normalise_reference(ob.data, ob.weight, ob.seg_first, nm)
    assert np.isfinite(mirror[0]).all()
    oc.check_normalised(E.normalise_observed(), mirror, "%d exposures, %s" % (nexp, "edge weights" if weighted else "no weights"))
    E.close()


# ---- 2. the detrending calls with a recipe installed -------------------------------------------------------------
@pytest.mark.parametrize("injected", [False, True])
@pytest.mark.parametrize("nm", [oc.MEDIAN_RATIO, xcor.Normalise(Q, DIVIDE, 0.9, 3.0), xcor.Normalise(NONE, SUBTRACT, 0.5, 0.0)], ids=nc.name)
def test_detrend_and_pca_run_step_1b(case, nm, injected):
    P = case.P
    ob = case.observed(12, True)
    shifts = np.array([pixels.shift(v) for v in np.linspace(-30.0, 30.0, 12)])
    E = case.handle(ob)
    f0, inject = ob.data, None
    if injected:
        pairs = E.run_pixels(P.atm, P.opts, shifts)
        inject = (P.atm, P.opts, shifts, 0.05 / case.scale, 0.9)
        f0 = xcor.inject_reference(pairs, ob, inject[3], inject[4])
        assert np.count_nonzero(f0 != ob.data) > 12 * 700
    E.set_normalise(nm)
    norm = xcor.normalise_reference(f0, ob.weight, ob.seg_first, nm)
    what = nc.name(nm) + (", injected" if injected else "")
    N = E.normalise_observed(inject=inject)
    oc.check_normalised(N, norm, what)
    assert (N.spectrum is None) == (not injected) and (not injected or np.array_equal(N.spectrum, case.spec))
    # SYSREM of the normalised data
    basis, coef, resid = xcor.sysrem_reference(norm[0], ob.weight, ob.seg_first, 3, 10)
    D = E.detrend_observed(3, 10, inject=inject)
    assert np.isfinite(basis).all() and np.isfinite(resid).all(), what
    assert same_bits(D.basis, basis) and same_bits(D.coef, coef) and same_bits(D.data, resid), what
    assert D.nsingular == oc.nsingular_of(ob, basis), what
    # PCA of the same
    basis, coef, resid, eigen, offdiag, nwhole = xcor.pca_reference(norm[0], ob.weight, ob.seg_first, 3, 8)
    D = E.pca_observed(3, 8, inject=inject)
    assert same_bits(D.basis, basis) and same_bits(D.coef, coef) and same_bits(D.data, resid), what
    assert same_bits(D.eigen, eigen) and same_bits(D.offdiag, offdiag) and np.array_equal(D.nwhole, nwhole), what
    # and they differ from the calls without the recipe
    E.set_normalise(None)
    assert not same_bits(E.detrend_observed(3, 10, inject=inject).data, resid)
    E.close()


# ---- 3. the state the three calls share ---------------------------------------------------------------------------
def test_the_three_calls_undo_one_another_and_start_from_raw(case):
    P = case.P
    ob = case.observed(7, True)
    E = case.handle(ob)
    fresh = E.run_moments(P.atm, P.opts, SHIFTS)
    E.set_normalise(oc.MEDIAN_RATIO)
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), fresh)        # installing the recipe changes nothing in force
    N1 = E.normalise_observed()
    oc.check_normalised(N1, xcor.normalise_reference(ob.data, ob.weight, ob.seg_first, oc.MEDIAN_RATIO), "first call")
    normalised = E.run_moments(P.atm, P.opts, SHIFTS)
    assert not same_bits(normalised, fresh)
    with pytest.raises(EngineError) as ei:                               # no filter after it
        E.run_filtered_moments(P.atm, P.opts, SHIFTS)
    assert ei.value.code == -1 and "no filter installed" in str(ei.value)
    D1 = E.detrend_observed(3, 10)
    assert not same_bits(D1.data, N1.data)
    E.run_filtered_moments(P.atm, P.opts, SHIFTS)                        # (the detrend's filter is in the slot)
    N2 = E.normalise_observed()
    assert same_bits(N2.data, N1.data) and same_bits(N2.rowscale, N1.rowscale) and same_bits(N2.centre, N1.centre) and (N2.nclipped, N2.nbad) == (N1.nclipped, N1.nbad)
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), normalised)
    with pytest.raises(EngineError):                                     # the filter slot is cleared again
        E.run_filtered_moments(P.atm, P.opts, SHIFTS)
    E.pca_observed(2, 8)
    quiet = E.normalise_observed(outputs=False)
    assert quiet.data is None and quiet.rowscale is None and quiet.centre is None and (quiet.nclipped, quiet.nbad) == (N1.nclipped, N1.nbad)
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), normalised)
    assert same_bits(E.detrend_observed(3, 10).data, D1.data)
    # detrend_observed(0) after normalise_observed restores the raw data
    E.normalise_observed()
    assert E.detrend_observed(0).nsingular == 0
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), fresh)
    # set_normalise(None): the parent's detrend bits, those of a handle that never had a recipe
    E.set_normalise(None)
    F = case.handle(ob)
    want, got = F.detrend_observed(3, 10), E.detrend_observed(3, 10)
    assert same_bits(got.basis, want.basis) and same_bits(got.coef, want.coef) and same_bits(got.data, want.data) and got.nsingular == want.nsingular
    basis, coef, resid = xcor.sysrem_reference(ob.data, ob.weight, ob.seg_first, 3, 10)
    assert same_bits(got.data, resid) and not same_bits(got.data, D1.data)
    want, got = F.pca_observed(3, 8), E.pca_observed(3, 8)
    assert same_bits(got.basis, want.basis) and same_bits(got.data, want.data) and same_bits(got.eigen, want.eigen)
    F.close()
    # set_observed drops the recipe
    E.set_normalise(oc.MEDIAN_RATIO)
    E.set_observed(ob)
    with pytest.raises(EngineError) as ei:
        E.normalise_observed()
    assert ei.value.code == -1 and "trx_normalise_observed: no recipe installed (trx_set_normalise)" in str(ei.value)
    assert same_bits(E.detrend_observed(3, 10).data, resid)
    E.set_normalise(oc.MEDIAN_RATIO)
    E.set_pixels(case.px)                                                # and so does set_pixels, with the observed set
    E.set_observed(ob)
    assert same_bits(E.detrend_observed(3, 10).data, resid)
    E.close()


def test_the_weights_in_force_and_the_calls_after_it(case):
    P = case.P
    ob = case.observed(12, True)
    V = _abi.SCATTER_VARIANCE
    hp = xcor.gaussian_highpass(6.0)
    nm = xcor.Normalise(Q, DIVIDE, 0.5, 3.0)
    shifts = np.array([pixels.shift(v) for v in np.linspace(-30.0, 30.0, 12)])
    norm = xcor.normalise_reference(ob.data, ob.weight, ob.seg_first, nm)[0]
    E = case.handle(ob)
    E.set_highpass(hp)
    E.set_normalise(nm)
    E.normalise_observed()
    installed = E.run_moments(P.atm, P.opts, shifts)                     # the normalised data under the installed weights
    # a weigh puts other weights in force; the next normalise puts the installed ones back
    R = E.weigh_observed(V, clip=3.0)
    var, med, keep, w1 = xcor.scatter_reference(norm, ob.weight, ob.seg_first, V, 3.0, 2)
    assert same_bits(R.variance, var) and same_bits(R.weight, w1)        # (the weigh read the normalised data)
    assert not same_bits(E.run_moments(P.atm, P.opts, shifts), installed)
    N = E.normalise_observed()
    assert same_bits(N.data, norm) and same_bits(E.run_moments(P.atm, P.opts, shifts), installed)
    # a later high-pass reads the normalised data, a weigh behind it the high-passed ones; the next normalise discards both
    H = E.highpass_observed()
    hp_data, ndead = xcor.highpass_observed_reference(norm, ob.weight, ob.seg_first, hp)
    assert same_bits(H.data, hp_data) and H.ndead == ndead
    R = E.weigh_observed(V, clip=3.0)
    assert same_bits(R.variance, xcor.scatter_reference(hp_data, ob.weight, ob.seg_first, V, 3.0, 2)[0])
    E.normalise_observed(outputs=False)
    assert same_bits(E.run_moments(P.atm, P.opts, shifts), installed)
    E.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------
def test_refusals_by_code_and_message_leave_everything_untouched(case):
    P = case.P
    ob = case.observed(7, True)
    E = case.handle(ob)
    E.set_normalise(oc.MEDIAN_RATIO)
    D = E.detrend_observed(3, 10)
    ref = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    who = "trx_set_normalise: "
    nan, inf = float("nan"), float("inf")
    for nm, text in ((xcor.Normalise(2, 4, nan, nan), "row_kind must be TRX_NORM_ROW_NONE or _QUANTILE"),
                     (xcor.Normalise(-1, 1), "row_kind must be TRX_NORM_ROW_NONE or _QUANTILE"),
                     (xcor.Normalise(1, 4, nan, nan), "col_kind must be TRX_NORM_COL_NONE, _DIVIDE, _RATIO or _SUBTRACT"),
                     (xcor.Normalise(0, -1, nan, nan), "col_kind must be TRX_NORM_COL_NONE, _DIVIDE, _RATIO or _SUBTRACT"),
                     (xcor.Normalise(0, 1, nan, nan), "quantile must be finite and in [0, 1]"),
                     (xcor.Normalise(0, 1, 1.5, nan), "quantile must be finite and in [0, 1]"),
                     (xcor.Normalise(1, 1, -0.1, -1.0), "quantile must be finite and in [0, 1]"),
                     (xcor.Normalise(1, 1, 0.5, inf), "clip must be finite"),
                     (xcor.Normalise(1, 1, 0.5, -1.0), "clip < 0"),
                     (xcor.Normalise(1, 1, 0.5, 0.5), "clip must be 0 (none) or at least 1"),
                     (xcor.Normalise(0, 0, 0.5, 0.0), "a recipe that does nothing (pass NULL to clear)")):
        with pytest.raises(EngineError) as ei:
            E.set_normalise(nm)
        assert ei.value.code == -1 and who + text in str(ei.value), (nm, str(ei.value))
    # the recipe, the data and the filter of the last good calls are in force
    after = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    assert same_bits(after[0], ref[0]) and same_bits(after[1], ref[1])
    assert same_bits(E.detrend_observed(3, 10).data, D.data)
    # trx_normalise_observed without a recipe: nothing touched, the outputs included
    E.set_normalise(None)
    after = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)   # (clearing the recipe is host work alone)
    assert same_bits(after[0], ref[0]) and same_bits(after[1], ref[1])
    lib, dp = E._lib, _abi.c_double_p
    data, scale, centre = np.full((7, 800), -7.0), np.full((7, 8), -7.0), np.full(800, -7.0)
    nclip, nbad = C.c_int64(-7), C.c_int64(-7)

    def raw(inject=0, p0=0.0):
        rc = lib.trx_normalise_observed(E._h, None, None, None, 0, None, inject, p0, 1.0, data.ctypes.data_as(dp), scale.ctypes.data_as(dp),
                                        centre.ctypes.data_as(dp), C.byref(nclip), C.byref(nbad), None)
        assert np.all(data == -7.0) and np.all(scale == -7.0) and np.all(centre == -7.0) and (nclip.value, nbad.value) == (-7, -7)
        return rc, E._last_error()

    run = "trx_normalise_observed: "
    assert raw() == (-1, run + "no recipe installed (trx_set_normalise)")
    assert raw(inject=2, p0=nan) == (-1, run + "no recipe installed (trx_set_normalise)")
    E.set_normalise(oc.MEDIAN_RATIO)
    assert raw(inject=2, p0=nan) == (-1, run + "inject must be 0 or 1")
    assert raw(inject=1, p0=nan) == (-1, run + "p0 must be finite")
    assert raw(inject=1) == (-1, run + "a is NULL")
    after = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    assert same_bits(after[0], ref[0]) and same_bits(after[1], ref[1])
    E.close()
    # no observed set
    N = case.handle(None)
    for nm in (oc.MEDIAN_RATIO, None):
        with pytest.raises(EngineError) as ei:
            N.set_normalise(nm)
        assert ei.value.code == -1 and who + "no observed set installed (trx_set_observed)" in str(ei.value)
    with pytest.raises(EngineError) as ei:
        N.normalise_observed()
    assert ei.value.code == -1 and run + "no observed set installed (trx_set_observed)" in str(ei.value)
    N.close()
    # a shard of the grid
    n = P.nwn
    try:
        P.set_shard(1000, 3000)
        S = Engine(P.static)
        S.set_pixels(pixels.Pixels([2510.0, 2520.0, 2530.0, 2540.0], [0.2, 0.3, 1.5, 0.4], 4.0))
        S.set_observed(xcor.Observed([0, 1, 4], np.ones((7, 4))))
        for nm in (oc.MEDIAN_RATIO, None):
            with pytest.raises(EngineError) as ei:
                S.set_normalise(nm)
            assert ei.value.code == -6 and who + "this handle's shard is not the whole grid" in str(ei.value)
        with pytest.raises(EngineError) as ei:                           # (no recipe can be installed on a shard: that comes first)
            S.normalise_observed()
        assert ei.value.code == -1 and run + "no recipe installed (trx_set_normalise)" in str(ei.value)
        assert S.run_pixels(P.atm, P.opts, SHIFTS).shape == (7, 4, 2)
        S.close()
    finally:
        P.set_shard(0, n)
