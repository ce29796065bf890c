"""Regressing the observed exposures on given time vectors on the device, with model injection (trx_regress_observed,
include/transit_hip.h), against transit_amd.xcor's mirrors of the same definition -- regress_reference, and for what follows
it inject_reference, normalise_reference, sysrem_reference, weighted_factor, highpass_observed_reference and
scatter_reference -- BIT FOR BIT.

The problem is observed_cases.build_case's: pixel_cases.make("eclipse", 20 000 lines, 6001 bins), the 800 pixels with their two off-grid ones,
the segments [1, 63, 64, 65, 200, 0, 7, 400], sysrem_cases' data at the model's scale and its edge weights (5 % single
masked entries, a column masked at every exposure, an exposure masked over a whole segment); the long orders are
many_cases.long_set's.  The vectors are regress_cases': the time basis of a synthetic airmass, seeded vectors behind it, and
vectors that differ from segment to segment.

The refusal of nexp * npix above what one pixel launch takes cannot be reached on a device; tests/regress_check.cpp holds
the refusals' text and order on the host."""
import ctypes as C

import numpy as np
import pytest

import many_cases as mc
import observed_cases as oc
import pixel_cases as pc
import regress_cases as rc
import sysrem_cases as sc
import xcor_checks as xc
from bits import same_bits
from transit_amd import _abi, broaden, pixels, xcor
from transit_amd.engine import Engine, EngineError
from transit_amd.exposures import Exposures

pytestmark = pytest.mark.gpu

SHIFTS = pc.SHIFTS
NSEG = len(sc.LENGTHS)
V = xcor.SCATTER_VARIANCE


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return oc.build_case(tmp_path_factory.mktemp("regress"), oc.SysremCase)


def everywhere(vec, nseg=NSEG):
    return np.ascontiguousarray(np.broadcast_to(vec[None, :, :], (nseg,) + vec.shape))


def mirror_of(f0, ob, vec, nfit=0, niter=10):
    """(basis, coef, resid, nsingular_fit, nsingular): the call's outputs in numpy from f0 and ob's weights"""
    vec = np.asarray(vec, dtype=np.float64)
    vec = everywhere(vec, ob.nseg) if vec.ndim == 2 else vec
    coef, resid, nfs = xcor.regress_reference(f0, ob.weight, ob.seg_first, vec)
    basis = vec
    if nfit:
        U, c, resid = xcor.sysrem_reference(resid, ob.weight, ob.seg_first, nfit, niter)
        basis, coef = np.concatenate([vec, U], axis=2), np.concatenate([coef, c], axis=0)
    return basis, coef, resid, nfs, oc.nsingular_of(ob, basis)


def check_outputs(D, mirror, what):
    basis, coef, resid, nfs, nsing = mirror
    assert np.isfinite(coef).all() and np.isfinite(resid).all(), what
    assert same_bits(D.basis, basis), what
    assert same_bits(D.coef, coef), what
    assert same_bits(D.data, resid), what
    assert (D.nsingular_fit, D.nsingular) == (nfs, nsing), what


def same_result(a, b):
    return (same_bits(a.basis, b.basis) and same_bits(a.coef, b.coef) and same_bits(a.data, b.data) and
            (a.nsingular_fit, a.nsingular) == (b.nsingular_fit, b.nsingular))


# ---- 1. bits without injection --------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nexp", [7, 12])
def test_bits_over_the_eight_orders(case, nexp, weighted):
    ob = case.observed(nexp, weighted)
    E = case.handle(ob)
    for nvec in (1, 3, 4, 5):
        what = "nexp %d, nvec %d, %s" % (nexp, nvec, "edge weights" if weighted else "no weights")
        vec = rc.given(nexp, nvec)
        D = E.regress_observed(vec)                            # [nexp, nvec]: the same vectors in every segment
        mirror = mirror_of(ob.data, ob, vec)
        check_outputs(D, mirror, what)
        assert D.spectrum is None and D.nsingular == D.nsingular_fit, what       # (nfit = 0: one factor, one count)
        if weighted:
            assert np.all(D.coef[:, sc.MASKED_COL] == 0) and np.array_equal(D.data[:, sc.MASKED_COL], ob.data[:, sc.MASKED_COL]), what
            assert D.nsingular >= 1, what
        else:
            assert D.nsingular == 0, what
        print("%s: basis, coef, data, nsingular_fit and nsingular (%d) are the mirror's" % (what, D.nsingular))
    E.close()


@pytest.mark.parametrize("weighted", [False, True])
def test_bits_at_every_padded_count(case, weighted):
    """nvec 1, 3, 5, 9 and 16 at 17 exposures: the kernels of 4, 8 and 16 padded components, 16 of them full"""
    nexp = rc.NEXP_16
    ob = case.observed(nexp, weighted)
    E = case.handle(ob)
    for nvec in (1, 3, 5, 9, 16):
        vec = rc.given(nexp, nvec)
        check_outputs(E.regress_observed(vec), mirror_of(ob.data, ob, vec), "17 exposures, nvec %d" % nvec)
    E.close()


@pytest.mark.parametrize("weighted", [False, True])
def test_bits_with_vectors_per_segment(case, weighted):
    ob = case.observed(12, weighted)
    vec = rc.per_segment(NSEG, 12, 5)
    E = case.handle(ob)
    D = E.regress_observed(vec)
    check_outputs(D, mirror_of(ob.data, ob, vec), "per-segment vectors")
    # (segment 0's vectors everywhere give other bits in every other segment: the mirror tells the two apart)
    wrong = xcor.regress_reference(ob.data, ob.weight, ob.seg_first, vec[0])[1]
    assert not same_bits(D.data[:, sc.SEG[7]:], wrong[:, sc.SEG[7]:])
    E.close()


@pytest.mark.parametrize("nexp", [64, 65])
def test_bits_about_a_whole_number_of_trips(case, nexp):
    """65 exposures are no multiple of the four whose loads a lane has in flight, 64 are"""
    ob = case.observed(nexp, True)
    vec = rc.given(nexp, 3)
    E = case.handle(ob)
    check_outputs(E.regress_observed(vec), mirror_of(ob.data, ob, vec), "%d exposures" % nexp)
    E.close()


def test_bits_on_the_long_orders(case):
    """many_cases.long_set: orders of 1024, 1025, 0, 2049 and 7 pixels"""
    ms = mc.long_set()[0]
    px = pixels.resolving_power(np.linspace(2503.0, 2557.0, ms.npix), 20000.0, 4.0)
    for p, c in ms.off_grid.items():
        px.centre[p] = c
    ob = ms.observed(case.scale, weighted=True)
    vec = rc.airmass_vectors(ms.nexp, 2)
    E = case.handle(ob, px)
    D = E.regress_observed(vec)
    check_outputs(D, mirror_of(ob.data, ob, vec), "long orders")
    assert D.nsingular_fit == 1                                # the column masked at every exposure
    E.close()


# ---- 2. injection: with a duplicated vector every column is singular, so the data ARE f0 -------------------------
@pytest.mark.parametrize("setup", ["table", "pixels", "table and broadening"])
def test_the_injected_data(case, setup):
    P = case.P
    ob = case.observed(7, True)
    E = case.handle(ob)
    if setup != "pixels":
        E.set_exposures(Exposures(xc.SCALE0.copy(), xc.SMEAR.copy()))
    if "broadening" in setup:
        E.set_broadening(broaden.Rotation(4.0, 0.4))
    E.set_highpass(xcor.gaussian_highpass(6.0))                # a high-pass takes no part in the injection
    pairs = E.run_exposed(P.atm, P.opts, SHIFTS) if setup != "pixels" else E.run_pixels(P.atm, P.opts, SHIFTS)
    p0, p1 = 0.05 / case.scale, 0.9
    f0 = xcor.inject_reference(pairs, ob, p0, p1)
    on = pairs[..., 1] > 0
    assert np.count_nonzero(on) > 7 * 700 and np.all(f0[on] != ob.data[on])
    dup = np.ones((7, 2))
    D = E.regress_observed(dup, inject=(P.atm, P.opts, SHIFTS, p0, p1))
    assert D.nsingular_fit == sc.NPIX == D.nsingular and np.all(D.coef == 0) and not np.signbit(D.coef).any()
    assert same_bits(D.data, f0), setup
    assert np.array_equal(D.spectrum, case.spec)               # run()'s bits, never the broadened spectrum
    # and a fit of the injected data
    vec = rc.airmass_vectors(7, 2)
    check_outputs(E.regress_observed(vec, inject=(P.atm, P.opts, SHIFTS, p0, p1)), mirror_of(f0, ob, vec), setup)
    E.close()


# ---- 3. behind a normalise recipe ---------------------------------------------------------------------------------
@pytest.mark.parametrize("injected", [False, True])
def test_behind_a_normalise_recipe(case, injected):
    P = case.P
    ob = case.observed(12, True)
    shifts = np.array([pixels.shift(v) for v in np.linspace(-30.0, 30.0, 12)])
    nm = xcor.Normalise(xcor.NORM_ROW_QUANTILE, xcor.NORM_COL_RATIO, 0.5, 0.0)
    E = case.handle(ob)
    f0, inject = ob.data, None
    if injected:
        inject = (P.atm, P.opts, shifts, 0.05 / case.scale, 0.9)
        f0 = xcor.inject_reference(E.run_pixels(P.atm, P.opts, shifts), ob, inject[3], inject[4])
    E.set_normalise(nm)
    norm = xcor.normalise_reference(f0, ob.weight, ob.seg_first, nm)[0]
    vec = rc.airmass_vectors(12, 2)
    D = E.regress_observed(vec, inject=inject)
    check_outputs(D, mirror_of(norm, ob, vec), "recipe" + (", injected" if injected else ""))
    E.set_normalise(None)
    assert not same_bits(E.regress_observed(vec, inject=inject).data, D.data)
    E.close()


# ---- 4. SYSREM components behind the given vectors ----------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_two_fitted_components_behind_the_given_vectors(case, weighted):
    ob = case.observed(12, weighted)
    vec = rc.airmass_vectors(12, 2)
    E = case.handle(ob)
    D = E.regress_observed(vec, nfit=2, niter=10)
    mirror = mirror_of(ob.data, ob, vec, 2, 10)
    check_outputs(D, mirror, "nfit = 2")
    assert D.basis.shape == (NSEG, 12, 5) and D.coef.shape == (5, sc.NPIX)
    assert same_bits(D.basis[..., :3], everywhere(vec))        # the given vectors, then SYSREM's of the regression's residuals
    resid0 = xcor.regress_reference(ob.data, ob.weight, ob.seg_first, vec)[1]
    U, c, resid = xcor.sysrem_reference(resid0, ob.weight, ob.seg_first, 2, 10)
    assert same_bits(D.basis[..., 3:], U) and same_bits(D.coef[3:], c) and same_bits(D.data, resid)
    assert D.nsingular >= D.nsingular_fit
    # one alternation, one component
    check_outputs(E.regress_observed(vec, nfit=1, niter=1), mirror_of(ob.data, ob, vec, 1, 1), "nfit = 1, niter = 1")
    E.close()


# ---- 5. the filter installed ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfit", [0, 2])
def test_the_filter_installed_is_the_weighted_filter_of_the_merged_basis(case, nfit):
    """run_filtered_moments after the call against a fresh handle's with set_observed(resid, W) and set_weighted_filter(B):
    with nfit = 0 the factor the fit ran from IS the installed filter's"""
    P = case.P
    ob = case.observed(7, True)
    vec = rc.airmass_vectors(7, 2)
    E = case.handle(ob)
    E.set_filter(xcor.svd_filter(ob.data, ob.seg_first, 2))    # a plain filter in the slot: replaced
    D = E.regress_observed(vec, nfit=nfit)
    basis, coef, resid, nfs, nsing = mirror_of(ob.data, ob, vec, nfit)
    check_outputs(D, (basis, coef, resid, nfs, nsing), "nfit %d" % nfit)
    got = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    F = case.handle(xcor.Observed(ob.seg_first, resid, ob.weight, ob.gain))
    assert F.set_weighted_filter(xcor.WeightedFilter(basis)) == D.nsingular
    want = F.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    F.close()
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert np.count_nonzero(np.isfinite(got[1]).all(axis=0)) > 700 and np.isnan(got[1][:, sc.MASKED_COL]).all()
    E.close()


# ---- 6. the state the four calls share ------------------------------------------------------------------------------
def test_from_raw_the_undo_and_the_other_calls(case):
    P = case.P
    ob = case.observed(7, True)
    vec = rc.airmass_vectors(7, 2)
    nm = xcor.Normalise(xcor.NORM_ROW_QUANTILE, xcor.NORM_COL_RATIO, 0.5, 0.0)
    E = case.handle(ob)
    fresh = E.run_moments(P.atm, P.opts, SHIFTS)
    undo = E.regress_observed(None)                            # nothing had been detrended: TRX_OK
    assert undo.data is None and (undo.nsingular_fit, undo.nsingular) == (0, 0) and same_bits(E.run_moments(P.atm, P.opts, SHIFTS), fresh)
    R1 = E.regress_observed(vec)
    check_outputs(R1, mirror_of(ob.data, ob, vec), "first call")
    regressed = E.run_moments(P.atm, P.opts, SHIFTS)
    assert not same_bits(regressed, fresh)
    assert same_result(E.regress_observed(vec), R1)            # twice: from raw, the same bits
    R2 = E.regress_observed(vec, nfit=2)
    assert not same_bits(R2.data, R1.data) and same_result(E.regress_observed(vec), R1)
    quiet = E.regress_observed(vec, outputs=False)
    assert quiet.basis is None and quiet.data is None and (quiet.nsingular_fit, quiet.nsingular) == (R1.nsingular_fit, R1.nsingular)
    mom = E.run_filtered_moments(P.atm, P.opts, SHIFTS)

    def undone():
        ok = same_bits(E.run_moments(P.atm, P.opts, SHIFTS), fresh)
        with pytest.raises(EngineError) as ei:
            E.run_filtered_moments(P.atm, P.opts, SHIFTS)
        return ok and ei.value.code == -1 and "no filter installed" in str(ei.value)

    # the undo by each of the four calls (normalise_observed has none of its own: detrend_observed(0) is its undo)
    assert E.regress_observed(np.zeros((7, 0))).nsingular == 0 and undone()
    E.regress_observed(vec)
    assert E.detrend_observed(0).nsingular == 0 and undone()
    E.regress_observed(vec)
    assert E.pca_observed(0).nsingular == 0 and undone()
    E.detrend_observed(3, 10)
    assert E.regress_observed(None).nsingular == 0 and undone()
    E.pca_observed(2, 8)
    assert E.regress_observed(None).nsingular == 0 and undone()
    E.set_normalise(nm)
    E.normalise_observed()
    assert E.regress_observed(None).nsingular == 0 and undone()
    E.set_normalise(None)
    assert same_result(E.regress_observed(vec), R1)
    assert same_bits(E.run_filtered_moments(P.atm, P.opts, SHIFTS), mom)
    # regress -> detrend and detrend -> regress: the second call has a fresh handle's bits
    F = case.handle(ob)
    want_d, want_p = F.detrend_observed(3, 10), F.pca_observed(2, 8)
    F.close()
    got = E.detrend_observed(3, 10)
    assert same_bits(got.basis, want_d.basis) and same_bits(got.coef, want_d.coef) and same_bits(got.data, want_d.data) and got.nsingular == want_d.nsingular
    assert same_result(E.regress_observed(vec), R1)
    got = E.pca_observed(2, 8)
    assert same_bits(got.basis, want_p.basis) and same_bits(got.data, want_p.data) and got.nsingular == want_p.nsingular
    assert same_result(E.regress_observed(vec, nfit=2), R2)
    # set_observed drops everything
    ob12 = case.observed(12, True)
    E.set_observed(ob12)
    with pytest.raises(EngineError):
        E.run_filtered_moments(P.atm, P.opts, np.full(12, SHIFTS[0]))
    vec12 = rc.airmass_vectors(12, 2)
    check_outputs(E.regress_observed(vec12), mirror_of(ob12.data, ob12, vec12), "after set_observed")
    E.close()


def test_the_highpass_and_the_weigh_after_it_and_the_weights_in_force(case):
    P = case.P
    ob = case.observed(12, True)
    vec = rc.airmass_vectors(12, 2)
    hp = xcor.gaussian_highpass(6.0)
    shifts = np.array([pixels.shift(v) for v in np.linspace(-30.0, 30.0, 12)])
    resid = xcor.regress_reference(ob.data, ob.weight, ob.seg_first, vec)[1]
    E = case.handle(ob)
    E.set_highpass(hp)
    E.regress_observed(vec)
    installed = E.run_filtered_moments(P.atm, P.opts, shifts)  # the residuals under the installed weights
    H = E.highpass_observed()
    hp_data, ndead = xcor.highpass_observed_reference(resid, ob.weight, ob.seg_first, hp)
    assert same_bits(H.data, hp_data) and H.ndead == ndead
    R = E.weigh_observed(V, clip=3.0)
    var, med, keep, w1 = xcor.scatter_reference(hp_data, ob.weight, ob.seg_first, V, 3.0, 2)
    assert same_bits(R.variance, var) and same_bits(R.median, med) and same_bits(R.weight, w1)
    assert not same_bits(E.run_filtered_moments(P.atm, P.opts, shifts), installed)
    # the next call discards the high-pass and puts the installed weights back in force, even after a weigh
    D = E.regress_observed(vec)
    assert same_bits(D.data, resid) and same_bits(E.run_filtered_moments(P.atm, P.opts, shifts), installed)
    E.weigh_observed(V, clip=3.0)
    E.regress_observed(vec, nfit=1, outputs=False)
    E.regress_observed(vec, outputs=False)
    assert same_bits(E.run_filtered_moments(P.atm, P.opts, shifts), installed)
    E.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_by_code_and_message_in_their_order(case):
    P = case.P
    ob = case.observed(7, True)
    E = case.handle(ob)
    p0 = 0.05 / case.scale
    good = rc.airmass_vectors(7, 2)
    D = E.regress_observed(good, inject=(P.atm, P.opts, SHIFTS, p0, 1.0))
    ref = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)

    lib, dp = E._lib, _abi.c_double_p
    basis, coef, data = np.full((8, 7, 16), -7.0), np.full((16, 800), -7.0), np.full((7, 800), -7.0)
    spec, nfs, ns = np.full(P.nwn, -7.0), C.c_int64(-7), C.c_int64(-7)
    bad_shift = SHIFTS.copy()
    bad_shift[4] = -1.0
    vec = everywhere(np.ascontiguousarray(rc.given(7, 16)))   # [8][7][16]: enough for every nvec
    vec3 = everywhere(good)
    nan_vec = vec3.copy()
    nan_vec[5, 2, 1] = np.nan
    nan_vec[6, 0, 0] = np.inf

    def raw(rg, a=P.atm, o=P.opts, nshift=7, shift=SHIFTS):
        rc_ = lib.trx_regress_observed(E._h, C.byref(a) if a is not None else None, C.byref(o) if o is not None else None, spec.ctypes.data_as(dp),
                                       nshift, shift.ctypes.data_as(dp) if shift is not None else None, C.byref(rg), basis.ctypes.data_as(dp),
                                       coef.ctypes.data_as(dp), data.ctypes.data_as(dp), C.byref(nfs), C.byref(ns), None)
        # a refusal touches no output
        assert np.all(basis == -7.0) and np.all(coef == -7.0) and np.all(data == -7.0) and np.all(spec == -7.0) and (nfs.value, ns.value) == (-7, -7)
        return rc_, E._last_error()

    def rg(v=vec3, **fields):
        r = _abi.TrxRegress(3, 0, 10, 1, p0, 1.0, v.ctypes.data_as(dp) if v is not None else None)
        for k, x in fields.items():
            setattr(r, k, x)
        return r

    who = "trx_regress_observed: "
    assert raw(rg(nvec=-1)) == (-1, who + "nvec < 0")
    assert raw(rg(vec, nvec=17)) == (-1, who + "nvec above TRX_FILTER_MAX (16)")
    assert raw(rg(nfit=-1)) == (-1, who + "nfit < 0")
    assert raw(rg(nfit=14)) == (-1, who + "nvec + nfit above TRX_FILTER_MAX (16)")
    assert raw(rg(nfit=2, niter=0)) == (-1, who + "niter < 1")
    assert raw(rg(nfit=2, niter=65)) == (-1, who + "niter above TRX_SYSREM_MAX_ITER (64)")
    assert raw(rg(None)) == (-1, who + "NULL vectors array")
    assert raw(rg(nan_vec)) == (-1, who + "segment 5: vectors entry must be finite")
    assert raw(rg(inject=2)) == (-1, who + "inject must be 0 or 1")
    assert raw(rg(p0=float("nan"))) == (-1, who + "p0 must be finite")
    assert raw(rg(p1=float("inf"))) == (-1, who + "p1 must be finite")
    assert raw(rg(), a=None) == (-1, who + "a is NULL")
    assert raw(rg(), o=None) == (-1, who + "o is NULL")
    assert raw(rg(), shift=None) == (-1, who + "shift is NULL")
    assert raw(rg(), nshift=6) == (-1, who + "nshift 6 is not the observed set's nexp 7")
    assert raw(rg(), shift=bad_shift) == (-1, who + "shift 4 must be finite and > 0")
    # the order: the first fault in the header's list is the one named
    assert raw(rg(None, nvec=17, nfit=-1, niter=0, inject=2), a=None) == (-1, who + "nvec above TRX_FILTER_MAX (16)")
    assert raw(rg(None, nfit=-1, niter=0, inject=2), a=None) == (-1, who + "nfit < 0")
    assert raw(rg(None, nfit=14, niter=0, inject=2), a=None) == (-1, who + "nvec + nfit above TRX_FILTER_MAX (16)")
    assert raw(rg(None, nfit=2, niter=0, inject=2), a=None) == (-1, who + "niter < 1")
    assert raw(rg(None, nfit=2, inject=2), a=None) == (-1, who + "NULL vectors array")
    assert raw(rg(nan_vec, inject=2), a=None) == (-1, who + "segment 5: vectors entry must be finite")
    assert raw(rg(niter=0, inject=2, p0=float("nan")), a=None) == (-1, who + "inject must be 0 or 1")      # (nfit = 0: niter is not read)
    # after the refusals: the data and the filter of the last good call
    after = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    assert same_bits(after[0], ref[0]) and same_bits(after[1], ref[1])
    assert same_result(E.regress_observed(good, inject=(P.atm, P.opts, SHIFTS, p0, 1.0)), D)
    with pytest.raises(ValueError):
        E.regress_observed(np.ones((6, 2)))
    E.close()
    # no observed set
    N = case.handle(None)
    for v in (np.ones((0, 1)), None):
        with pytest.raises(EngineError) as ei:
            N.regress_observed(v)
        assert ei.value.code == -1 and who + "no observed set installed (trx_set_observed)" in str(ei.value)
    N.close()
    # a shard of the grid
    n = P.nwn
    try:
        P.set_shard(1000, 3000)
        S = Engine(P.static)
        S.set_pixels(pixels.Pixels([2510.0, 2520.0, 2530.0, 2540.0], [0.2, 0.3, 1.5, 0.4], 4.0))
        S.set_observed(xcor.Observed([0, 1, 4], np.ones((7, 4))))
        for inject in (None, (P.atm, P.opts, SHIFTS, p0, 1.0)):
            with pytest.raises(EngineError) as ei:
                S.regress_observed(np.ones((7, 1)), inject=inject)
            assert ei.value.code == -6 and who + "this handle's shard is not the whole grid" in str(ei.value)
        assert S.run_pixels(P.atm, P.opts, SHIFTS).shape == (7, 4, 2)
        S.close()
    finally:
        P.set_shard(0, n)


# ---- 8. injection and recovery, end to end ------------------------------------------------------------------------
def test_injection_and_recovery_end_to_end(case):
    """regress_cases.trend_set: a continuum whose columns change in time by their own multiples of the airmass powers, plus
    1e-4 of noise, two segments.  The model is injected with p0 = 0.1 / scale and p1 = 1 at the cell (Kp, Vsys) = (100, 6)
    km/s of test_gpu_trail's 5 x 5 map; the chain is regress_observed(time_basis(airmass, 2), nfit=2), weigh_observed(clip=3),
    run_exposed_map.  The strength is test_gpu_sysrem's and test_gpu_hpdata's; the numpy mirror chain -- run first, from the
    device's pixel pairs -- finds the injected cell with it and does not without the injection (its peak and runner-up are in
    docs/history.md).  Every step of the device chain is then in the mirror's bits."""
    P = case.P
    data, w, gain = rc.trend_set(7)
    seg = rc.E2E_SEG
    ob = xcor.Observed(seg, case.scale * data, w, gain)
    vec = xcor.time_basis(rc.airmass(7), 2)
    vm = xc.the_map("ccf", kp=xc.TRAIL_KP, vsys=xc.TRAIL_VSYS)
    cell = (int(np.argmin(np.abs(xc.TRAIL_KP - xc.KP_TRUE))), int(np.argmin(np.abs(xc.TRAIL_VSYS - xc.VSYS_TRUE))))
    assert cell == (2, 3) and (vm.nkp, vm.nvsys) == (5, 5)
    shifts = np.array([pixels.shift(v) for v in xc.VSYS_TRUE + xc.KP_TRUE * xc.ORBIT])
    p0 = 0.1 / case.scale
    E = case.handle(ob)
    E.set_exposures(Exposures(np.ones(7), np.full(7, 2e-6)))

    def peak(m):
        assert np.isfinite(m).all()
        return tuple(int(i) for i in np.unravel_index(np.argmax(m), m.shape))

    injected = E.run_exposed(P.atm, P.opts, shifts)
    pairs_lv = np.stack([E.run_exposed(P.atm, P.opts, np.full(7, s)) for s in xc.LAGS])

    def host_map(f0):
        basis, coef, resid, nfs, nsing = mirror_of(f0, ob, vec, 2, 10)
        var, med, keep, w1 = xcor.scatter_reference(resid, w, seg, V, 3.0, 2)
        return xcor.exposed_map_reference(pairs_lv, xcor.Observed(seg, resid, w1, gain), xcor.WeightedFilter(basis), vm), (basis, coef, resid, nfs, nsing, var, med, w1)

    (with_injection, mirror), (without, _) = host_map(xcor.inject_reference(injected, ob, p0, 1.0)), host_map(ob.data)
    order = np.sort(with_injection.reshape(-1))
    print("numpy chain, injected (rows Kp, columns Vsys):\n%s\nnumpy chain, not injected:\n%s\nnumpy chain: peak %.6e, runner-up %.6e"
          % (np.array2string(with_injection, precision=4), np.array2string(without, precision=4), order[-1], order[-2]))
    assert peak(with_injection) == cell and peak(without) != cell
    # the device
    D = E.regress_observed(vec, nfit=2, inject=(P.atm, P.opts, shifts, p0, 1.0))
    check_outputs(D, mirror[:5], "end to end")
    R = E.weigh_observed(V, clip=3.0)
    assert same_bits(R.variance, mirror[5]) and same_bits(R.median, mirror[6]) and same_bits(R.weight, mirror[7])
    m, idx = E.run_exposed_map(P.atm, P.opts, vm, lag_index=True)
    print("device (rows Kp, columns Vsys):\n%s" % np.array2string(m, precision=4))
    assert np.array_equal(idx, xcor.nearest_lags(vm)) and np.all(idx >= 0)
    assert peak(m) == cell
    for i in range(5):
        for j in range(5):
            mom = E.run_filtered_moments(P.atm, P.opts, xc.LAGS[idx[i, j]])
            want = xcor.cell_value(mom, vm)
            assert same_bits(m[i, j], want), (i, j, m[i, j], want)
    E.close()
