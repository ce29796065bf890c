"""The principal-component detrend of the observed exposures on the device, with model injection (trx_pca_observed,
include/transit_hip.h), against transit_amd.xcor's mirrors of the same definition -- inject_reference, pca_reference and, for
what the call installs, weighted_factor -- BIT FOR BIT: basis, coef, data, eigen, offdiag, nwhole and nsingular.

The case is observed_cases.build_case's: pixel_cases.make("eclipse", 20 000 lines, 6001 bins), the 800 pixels with their two off-grid ones,
the segments [1, 63, 64, 65, 200, 0, 7, 400], 7 and 12 exposures, sysrem_cases' data and edge weights.  Past one wave of
Jacobi pairs and at the cap -- 65, 100 and 128 exposures -- the set is two short segments of 130 and 64 pixels."""
import ctypes as C
import time

import numpy as np
import pytest

import observed_cases as oc
import pixel_cases as pc
import sysrem_cases as sc
import xcor_checks as xc
from bits import same_bits
from transit_amd import _abi, broaden, pixels, xcor
from transit_amd.engine import Engine, EngineError
from transit_amd.exposures import Exposures

pytestmark = pytest.mark.gpu

SHIFTS = pc.SHIFTS
V = xcor.SCATTER_VARIANCE


class Case(oc.SysremCase):
    def mirror(self, nexp, weighted, ncomp, nsweep):
        """xcor.pca_reference of the raw set, made once"""
        ob = self.observed(nexp, weighted)
        return self.memo((nexp, weighted, ncomp, nsweep), lambda: xcor.pca_reference(ob.data, ob.weight, ob.seg_first, ncomp, nsweep))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return oc.build_case(tmp_path_factory.mktemp("pca"), Case)


def same_result(a, b):
    return (same_bits(a.basis, b.basis) and same_bits(a.coef, b.coef) and same_bits(a.data, b.data) and same_bits(a.eigen, b.eigen) and
            same_bits(a.offdiag, b.offdiag) and np.array_equal(a.nwhole, b.nwhole) and a.nsingular == b.nsingular)


# ---- 1. bits without injection --------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ncomp", [1, 3, 5])
@pytest.mark.parametrize("nexp", [7, 12])
def test_bits_without_injection(case, nexp, ncomp, weighted):
    ob = case.observed(nexp, weighted)
    E = case.handle(ob)
    for nsweep in (1, 8):
        what = "nexp %d, ncomp %d, nsweep %d, %s" % (nexp, ncomp, nsweep, "edge weights" if weighted else "no weights")
        D = E.pca_observed(ncomp, nsweep)
        mirror = case.mirror(nexp, weighted, ncomp, nsweep)
        oc.check_pca_outputs(D, mirror, ob, what)
        assert D.spectrum is None
        basis = mirror[0]
        # the edges: the empty segment's vectors are zero, every other segment has a first component
        assert np.all(basis[5] == 0) and np.all(np.any(basis[[0, 1, 2, 3, 4, 6, 7], :, 0] != 0, axis=1)), what
        if weighted:
            k = slice(sc.SEG[sc.MASKED_SEG], sc.SEG[sc.MASKED_SEG + 1])
            assert np.all(D.basis[sc.MASKED_SEG, sc.MASKED_EXP] == 0) and not np.signbit(D.basis[sc.MASKED_SEG, sc.MASKED_EXP]).any(), what
            assert np.array_equal(D.data[sc.MASKED_EXP, k], ob.data[sc.MASKED_EXP, k]), what
            assert np.all(D.coef[:, sc.MASKED_COL] == 0) and np.array_equal(D.data[:, sc.MASKED_COL], ob.data[:, sc.MASKED_COL]), what
            assert D.nsingular >= 1 and 0 < D.nwhole[7] < 400, what
        else:
            assert np.array_equal(D.nwhole, sc.LENGTHS), what
        print("%s: basis, coef, data, eigen, offdiag, nwhole and nsingular (%d) are the mirror's" % (what, D.nsingular))
    E.close()


# ---- 2. past one wave of pairs, and at the cap --------------------------------------------------------------------
SHORT = xcor.segments([130, 64])


def short_set(case, nexp):
    """two short segments, smooth trends plus seeded noise at the model's scale; weights with 2 % single masked entries, a
    column masked at every exposure and an exposure masked over the whole second segment"""
    rng = np.random.default_rng(300 + nexp)
    npix = int(SHORT[-1])
    x, t = np.linspace(0.0, 1.0, npix), np.linspace(-1.0, 1.0, nexp)
    d = 1.0 + 0.3 * np.sin(7.0 * x)[None, :] * np.ones((nexp, 1))
    for k in range(6):
        d += 0.2 * 0.4 ** k * rng.uniform(-1.0, 1.0, nexp)[:, None] * np.cos((3.0 + 5.0 * k) * x + rng.uniform(0, 6.0))[None, :] * (1.0 + 0.2 * t[:, None])
    d += 0.01 * rng.standard_normal((nexp, npix))
    w = rng.uniform(0.5, 2.0, (nexp, npix))
    w[rng.random((nexp, npix)) < 0.02] = 0.0
    w[:, 40] = 0.0
    w[3, 130:] = 0.0
    px = pixels.resolving_power(np.linspace(2503.0, 2557.0, npix), 20000.0, 4.0)
    return px, xcor.Observed(SHORT, case.scale * d, w, rng.uniform(0.5, 1.5, npix))


@pytest.mark.parametrize("nexp,ncomp", [(65, 5), (100, 5), (128, 16)])
def test_many_exposures(case, nexp, ncomp):
    px, ob = short_set(case, nexp)
    E = case.handle(ob, px)
    D = E.pca_observed(ncomp, 8)
    mirror = xcor.pca_reference(ob.data, ob.weight, ob.seg_first, ncomp, 8)
    oc.check_pca_outputs(D, mirror, ob, "nexp %d" % nexp)
    assert np.all(D.basis[1, 3] == 0) and not np.signbit(D.basis[1, 3]).any() and np.all(D.coef[:, 40] == 0)
    assert 0 < D.nwhole[0] < 130 and 0 < D.nwhole[1] < 64 and np.all(D.eigen[:, 0] > 0)
    print("nexp %d, %d components: the mirror's; nwhole %s, offdiag / eigen[:, 0] %s" % (nexp, ncomp, D.nwhole, D.offdiag / D.eigen[:, 0]))
    E.close()


def test_above_the_cap_is_refused(case):
    px, ob = short_set(case, 129)
    E = case.handle(ob, px)
    with pytest.raises(EngineError) as ei:
        E.pca_observed(3)
    assert ei.value.code == -1 and "trx_pca_observed: the observed set's nexp 129 is above TRX_PCA_MAX_EXP (128)" in str(ei.value)
    assert E.pca_observed(0).nsingular == 0                  # the undo is the undo
    assert E.detrend_observed(1, 1).basis.shape == (2, 129, 1)      # SYSREM takes the set
    E.close()


# ---- 3. bits with injection -----------------------------------------------------------------------------------
@pytest.mark.parametrize("setup", ["table", "pixels", "table and broadening"])
def test_bits_with_injection(case, setup):
    P = case.P
    ob = case.observed(7, True)
    E = case.handle(ob)
    if setup != "pixels":
        E.set_exposures(Exposures(xc.SCALE0.copy(), xc.SMEAR.copy()))
    if "broadening" in setup:
        E.set_broadening(broaden.Rotation(4.0, 0.4))
    # a high-pass takes no part in the injection: the pairs are the ones ahead of it
    E.set_highpass(xcor.gaussian_highpass(6.0))
    pairs = E.run_exposed(P.atm, P.opts, SHIFTS) if setup != "pixels" else E.run_pixels(P.atm, P.opts, SHIFTS)
    p0, p1 = 0.05 / case.scale, 0.9
    f0 = xcor.inject_reference(pairs, ob, p0, p1)
    on = pairs[..., 1] > 0
    assert np.count_nonzero(on) > 7 * 700 and np.all(f0[on] != ob.data[on])
    # the data before the PCA are inject_reference's: the mirror starts from f0, and the masked column below keeps f0's bits
    # (test_the_injected_data_are_inject_references reads them off a whole set)
    mirror = xcor.pca_reference(f0, ob.weight, ob.seg_first, 3, 8)
    D = E.pca_observed(3, 8, inject=(P.atm, P.opts, SHIFTS, p0, p1))
    oc.check_pca_outputs(D, mirror, ob, setup)
    assert np.array_equal(D.spectrum, case.spec)             # run()'s bits, never the broadened spectrum
    assert same_bits(D.data[:, sc.MASKED_COL], f0[:, sc.MASKED_COL])     # a masked column keeps the injected data
    assert not same_bits(D.data, case.mirror(7, True, 3, 8)[2])
    # p0 = 0, p1 = 1 injects nothing
    D0 = E.pca_observed(3, 8, inject=(P.atm, P.opts, SHIFTS, 0.0, 1.0))
    oc.check_pca_outputs(D0, case.mirror(7, True, 3, 8), ob, setup + ", p0 = 0 and p1 = 1")
    E.close()


def test_the_injected_data_are_inject_references(case):
    """a set whose every column has a hole: no column is whole, every vector is zero, and the residuals are f0 itself"""
    P = case.P
    full = case.observed(7, True)
    w = np.ones((7, sc.NPIX))
    w[np.arange(sc.NPIX) % 7, np.arange(sc.NPIX)] = 0.0
    w[:, 0] = [0, 0, 1, 1, 1, 1, 1]                          # (the one-pixel segment: a hole at a live exposure needs two)
    w[0, 0] = 0.0
    ob = xcor.Observed(sc.SEG, full.data, w, full.gain)
    E = case.handle(ob)
    pairs = E.run_pixels(P.atm, P.opts, SHIFTS)
    f0 = xcor.inject_reference(pairs, ob, 0.05 / case.scale, 0.9)
    D = E.pca_observed(3, 2, inject=(P.atm, P.opts, SHIFTS, 0.05 / case.scale, 0.9))
    assert np.all(D.nwhole[1:] == 0) and np.all(D.basis[1:] == 0) and same_bits(D.data[:, 1:], f0[:, 1:])
    oc.check_pca_outputs(D, xcor.pca_reference(f0, w, sc.SEG, 3, 2), ob, "every column with a hole")
    E.close()


# ---- 4. sequences: twice, the undo by either call, the other detrend, the calls after it ----------------------------
def test_sequences_with_detrend_observed(case):
    P = case.P
    ob = case.observed(7, True)
    E = case.handle(ob)
    fresh = E.run_moments(P.atm, P.opts, SHIFTS)
    undo = E.pca_observed(0)                                 # nothing had been detrended: TRX_OK
    assert undo.data is None and undo.eigen is None and undo.nsingular == 0 and same_bits(E.run_moments(P.atm, P.opts, SHIFTS), fresh)
    P1 = E.pca_observed(3, 8)
    oc.check_pca_outputs(P1, case.mirror(7, True, 3, 8), ob, "first call")
    assert not same_bits(E.run_moments(P.atm, P.opts, SHIFTS), fresh)
    assert same_result(E.pca_observed(3, 8), P1)             # twice
    mom = E.run_filtered_moments(P.atm, P.opts, SHIFTS)
    S1 = E.detrend_observed(3, 10)                           # pca -> detrend: a fresh detrend's bits
    F = case.handle(ob)
    S0 = F.detrend_observed(3, 10)
    assert oc.same_detrend(S1, S0) and S1.eigen is None
    assert same_result(F.pca_observed(3, 8), P1)             # detrend -> pca: a fresh pca's bits
    F.close()
    assert same_result(E.pca_observed(3, 8), P1)
    assert same_bits(E.run_filtered_moments(P.atm, P.opts, SHIFTS), mom)
    quiet = E.pca_observed(3, 8, outputs=False)
    assert quiet.basis is None and quiet.eigen is None and quiet.nwhole is None and quiet.nsingular == P1.nsingular
    # the undo by either call
    assert E.detrend_observed(0).nsingular == 0
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), fresh)
    with pytest.raises(EngineError) as ei:
        E.run_filtered_moments(P.atm, P.opts, SHIFTS)
    assert ei.value.code == -1 and "no filter installed" in str(ei.value)
    E.detrend_observed(3, 10)
    assert E.pca_observed(0).nsingular == 0
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), fresh)
    with pytest.raises(EngineError):
        E.run_filtered_moments(P.atm, P.opts, SHIFTS)
    assert same_result(E.pca_observed(3, 8), P1)
    E.close()


def test_highpass_weigh_and_what_is_installed(case):
    P = case.P
    ob = case.observed(7, True)
    hp, ex = xcor.gaussian_highpass(6.0), Exposures(xc.SCALE0.copy(), xc.SMEAR.copy())
    E = case.handle(ob)
    E.set_filter(xcor.svd_filter(ob.data, ob.seg_first, 2))  # a plain filter in the slot: replaced
    E.set_highpass(hp)
    E.set_exposures(ex)
    E.highpass_observed()                                    # a high-pass over the raw data: the PCA uncovers it
    D = E.pca_observed(3, 8)
    basis, coef, resid, eigen, offdiag, nwhole = case.mirror(7, True, 3, 8)
    oc.check_pca_outputs(D, case.mirror(7, True, 3, 8), ob, "behind a high-pass and a table")
    # run_filtered_moments is a fresh handle's under the same residuals, weights and basis
    got = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    F = case.handle(xcor.Observed(ob.seg_first, resid, ob.weight, ob.gain))
    assert F.set_weighted_filter(xcor.WeightedFilter(basis)) == D.nsingular
    F.set_highpass(hp)
    F.set_exposures(ex)
    want = F.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert np.count_nonzero(np.isfinite(got[1]).all(axis=0)) > 700 and np.isnan(got[1][:, sc.MASKED_COL]).all()
    # pca -> highpass_observed -> weigh_observed: the mirrors' bits on the mirror's residuals
    H = E.highpass_observed()
    hp_want, ndead = xcor.highpass_observed_reference(resid, ob.weight, ob.seg_first, hp)
    assert same_bits(H.data, hp_want) and H.ndead == ndead
    Wg = E.weigh_observed(V, clip=3.0)
    var, med, keep, w1 = xcor.scatter_reference(hp_want, ob.weight, ob.seg_first, V, 3.0, 2)
    assert same_bits(Wg.variance, var) and same_bits(Wg.median, med) and same_bits(Wg.weight, w1)
    got = E.run_filtered_moments(P.atm, P.opts, SHIFTS)
    F.highpass_observed()
    F.weigh_observed(V, clip=3.0)
    assert same_bits(got, F.run_filtered_moments(P.atm, P.opts, SHIFTS))
    F.close()
    # and a second PCA starts from the raw data and the weights as installed
    assert same_result(E.pca_observed(3, 8), D)
    E.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(case):
    P = case.P
    ob = case.observed(7, True)
    E = case.handle(ob)
    p0 = 0.05 / case.scale
    D = E.pca_observed(3, 8, inject=(P.atm, P.opts, SHIFTS, p0, 1.0))
    ref = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    lib, dp = E._lib, _abi.c_double_p
    basis, coef, data = np.full((8, 7, 3), -7.0), np.full((3, 800), -7.0), np.full((7, 800), -7.0)
    eigen, off, nwh = np.full((8, 3), -7.0), np.full(8, -7.0), np.full(8, -7, dtype=np.int64)
    spec, ns = np.full(P.nwn, -7.0), C.c_int64(-7)
    bad_shift = SHIFTS.copy()
    bad_shift[4] = -1.0

    def raw(pc, a=P.atm, o=P.opts, nshift=7, shift=SHIFTS):
        rc = lib.trx_pca_observed(E._h, C.byref(a) if a is not None else None, C.byref(o) if o is not None else None, spec.ctypes.data_as(dp),
                                  nshift, shift.ctypes.data_as(dp) if shift is not None else None, C.byref(pc), basis.ctypes.data_as(dp),
                                  coef.ctypes.data_as(dp), data.ctypes.data_as(dp), eigen.ctypes.data_as(dp), off.ctypes.data_as(dp),
                                  nwh.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(ns), None)
        # a refusal touches no output
        assert np.all(basis == -7.0) and np.all(coef == -7.0) and np.all(data == -7.0) and np.all(spec == -7.0) and ns.value == -7
        assert np.all(eigen == -7.0) and np.all(off == -7.0) and np.all(nwh == -7)
        return rc, E._last_error()

    def pc(**fields):
        d = _abi.TrxPca(3, 8, 1, 0, p0, 1.0)
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    who = "trx_pca_observed: "
    assert raw(pc(ncomp=-1)) == (-1, who + "ncomp < 0")
    assert raw(pc(ncomp=17)) == (-1, who + "ncomp above TRX_FILTER_MAX (16)")
    assert raw(pc(ncomp=8)) == (-1, who + "ncomp 8 is above the observed set's nexp 7")
    assert raw(pc(nsweep=0)) == (-1, who + "nsweep < 1")
    assert raw(pc(nsweep=33)) == (-1, who + "nsweep above TRX_PCA_MAX_SWEEP (32)")
    assert raw(pc(inject=2)) == (-1, who + "inject must be 0 or 1")
    assert raw(pc(pad=1)) == (-1, who + "pad must be 0")
    assert raw(pc(p0=float("nan"))) == (-1, who + "p0 must be finite")
    assert raw(pc(p1=float("inf"))) == (-1, who + "p1 must be finite")
    assert raw(pc(), a=None) == (-1, who + "a is NULL")
    assert raw(pc(), o=None) == (-1, who + "o is NULL")
    assert raw(pc(), shift=None) == (-1, who + "shift is NULL")
    assert raw(pc(), nshift=6) == (-1, who + "nshift 6 is not the observed set's nexp 7")
    assert raw(pc(), shift=bad_shift) == (-1, who + "shift 4 must be finite and > 0")
    # the order: the first fault in the header's list is the one named
    assert raw(pc(ncomp=17, nsweep=0, inject=2, pad=1), a=None) == (-1, who + "ncomp above TRX_FILTER_MAX (16)")
    assert raw(pc(nsweep=33, pad=1, p0=float("nan")), shift=None) == (-1, who + "nsweep above TRX_PCA_MAX_SWEEP (32)")
    # after the refusals: the data and the filter of the last good call
    after = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    assert same_bits(after[0], ref[0]) and same_bits(after[1], ref[1])
    assert same_result(E.pca_observed(3, 8, inject=(P.atm, P.opts, SHIFTS, p0, 1.0)), D)
    E.close()
    # no observed set
    N = case.handle(None)
    for ncomp in (3, 0):
        with pytest.raises(EngineError) as ei:
            N.pca_observed(ncomp)
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
                S.pca_observed(1, 2, inject=inject)
            assert ei.value.code == -6 and who + "this handle's shard is not the whole grid" in str(ei.value)
        S.close()
    finally:
        P.set_shard(0, n)


# ---- 6. injection and recovery, end to end -----------------------------------------------------------------------
def test_injection_and_recovery_end_to_end(case):
    """test_gpu_sysrem's end-to-end set: a continuum with smooth trends in time plus seeded noise, two segments.  The model
    is injected with p1 = 1 at the cell (Kp, Vsys) = (100, 6) km/s of test_gpu_trail's 5 x 5 map, the PCA takes three
    components, the columns are weighed by their inverse variance with a clip of 3, and the CCF map of trx_run_exposed_map
    is the recovery."""
    P = case.P
    rng = np.random.default_rng(21)
    seg = xcor.segments([400, 400])
    x, t = np.linspace(0.0, 1.0, 800), np.linspace(-1.0, 1.0, 7)
    trend = (1.0 + 0.3 * np.sin(5.0 * x))[None, :] * (1.0 + 0.1 * t[:, None] + 0.05 * (t ** 2)[:, None] * np.cos(3.0 * x)[None, :])
    raw = case.scale * (trend + 1e-4 * rng.standard_normal((7, 800)))
    w = rng.uniform(0.5, 2.0, (7, 800))
    w[rng.random((7, 800)) < 0.02] = 0.0
    ob = xcor.Observed(seg, raw, w, rng.uniform(0.5, 1.5, 800))
    vm = xc.the_map("ccf", kp=xc.TRAIL_KP, vsys=xc.TRAIL_VSYS)
    cell = (int(np.argmin(np.abs(xc.TRAIL_KP - xc.KP_TRUE))), int(np.argmin(np.abs(xc.TRAIL_VSYS - xc.VSYS_TRUE))))
    assert cell == (2, 3) and (vm.nkp, vm.nvsys) == (5, 5)
    shifts = np.array([pixels.shift(v) for v in xc.VSYS_TRUE + xc.KP_TRUE * xc.ORBIT])
    p0 = 0.1 / case.scale
    E = case.handle(ob)
    E.set_exposures(Exposures(np.ones(7), np.full(7, 2e-6)))
    D = E.pca_observed(3, 8, inject=(P.atm, P.opts, shifts, p0, 1.0))
    f0 = xcor.inject_reference(E.run_exposed(P.atm, P.opts, shifts), ob, p0, 1.0)
    mirror = xcor.pca_reference(f0, w, seg, 3, 8)
    oc.check_pca_outputs(D, mirror, ob, "end to end")
    R = E.weigh_observed(V, clip=3.0)
    var, med, keep, w1 = xcor.scatter_reference(mirror[2], w, seg, V, 3.0, 2)
    assert same_bits(R.weight, w1)
    m, idx = E.run_exposed_map(P.atm, P.opts, vm, lag_index=True)
    print("device (rows Kp, columns Vsys):\n%s\nnwhole %s, %d columns clipped" % (np.array2string(m, precision=4), D.nwhole, R.nmasked))
    assert np.array_equal(idx, xcor.nearest_lags(vm)) and np.all(idx >= 0) and np.isfinite(m).all()
    assert tuple(int(i) for i in np.unravel_index(np.argmax(m), m.shape)) == cell
    # every cell has the bits of the same handle's filtered moments at the cell's lags
    for i in range(5):
        for j in range(5):
            mom = E.run_filtered_moments(P.atm, P.opts, xc.LAGS[idx[i, j]])
            want = xcor.cell_value(mom, vm)
            assert same_bits(m[i, j], want), (i, j, m[i, j], want)
    E.close()


# ---- 7. size and time --------------------------------------------------------------------------------------------
def test_size_and_time(case):
    """40 orders of 2048 pixels, 100 exposures, 5 components of 8 sweeps, 2 % of the columns masked: determinism and
    finiteness are asserted, the times are printed (a host clock around calls that return synchronised, after one warm-up
    call, the mean of 20) beside the host path the call replaces -- xcor.svd_basis plus the subtraction -- and
    detrend_observed(5, 10) in the same run.  The one assertion on time: the device call is faster than that host path."""
    P = case.P
    nseg, n, nexp, ncomp, nsweep, reps = 40, 2048, 100, 5, 8, 20
    npix = nseg * n
    px = pixels.resolving_power(np.linspace(2503.0, 2557.0, npix), 20000.0, 4.0)
    rng = np.random.default_rng(5)
    seg = xcor.segments([n] * nseg)
    x, t = np.linspace(0.0, 1.0, npix), np.linspace(-1.0, 1.0, nexp)
    raw = (1.0 + 0.3 * np.sin(40.0 * x))[None, :] * (1.0 + 0.05 * t[:, None] * np.sin(9.0 * x)[None, :] + 0.02 * (t ** 2)[:, None])
    raw = case.scale * (raw + 1e-3 * rng.standard_normal((nexp, npix)))
    w = rng.uniform(0.5, 2.0, (nexp, npix))
    w[:, rng.random(npix) < 0.02] = 0.0
    ob = xcor.Observed(seg, raw, w)
    shifts = np.array([pixels.shift(v) for v in np.linspace(-40.0, 40.0, nexp)])
    E = Engine(P.static)
    E.set_pixels(px)
    E.set_observed(ob)
    out, left = {}, {}
    for name, inject in (("pca_observed without injection", None), ("pca_observed with injection", (P.atm, P.opts, shifts, 0.05 / case.scale, 1.0))):
        first = E.pca_observed(ncomp, nsweep, inject=inject)                # (the warm-up)
        t0 = time.perf_counter()
        for _ in range(reps):
            E.pca_observed(ncomp, nsweep, inject=inject, outputs=False)
        out[name] = (time.perf_counter() - t0) / reps
        again = E.pca_observed(ncomp, nsweep, inject=inject)
        assert same_result(first, again), name
        assert np.isfinite(first.basis).all() and np.isfinite(first.coef).all() and np.isfinite(first.data).all(), name
        assert first.basis.shape == (nseg, nexp, ncomp) and np.all(np.abs(np.linalg.norm(first.basis, axis=1) - 1.0) < 1e-12), name
        assert np.all(first.nwhole > 1900) and np.all(first.eigen[:, 0] > 0), name
        left[name] = float(np.max(first.offdiag / first.eigen[:, 0]))
    E.detrend_observed(ncomp, 10)
    t0 = time.perf_counter()
    for _ in range(reps):
        E.detrend_observed(ncomp, 10, outputs=False)
    out["detrend_observed(5, 10)"] = (time.perf_counter() - t0) / reps
    E.close()
    t0 = time.perf_counter()
    host = xcor.svd_basis(raw, seg, ncomp)
    resid = raw.copy()
    for s in range(nseg):
        k = slice(s * n, (s + 1) * n)
        resid[:, k] -= host[s] @ (host[s].T @ raw[:, k])
    out["xcor.svd_basis and the subtraction on the host"] = time.perf_counter() - t0
    assert np.isfinite(host).all() and np.isfinite(resid).all()
    print("40 x 2048 pixels, 100 exposures, %d components, %d sweeps:" % (ncomp, nsweep))
    for name, s in out.items():
        print("  %-50s %9.3f ms" % (name, 1e3 * s))
    for name, x in left.items():
        print("  %s: the largest offdiag / eigen[:, 0] the 8 sweeps leave %.2e" % (name, x))
    assert out["pca_observed without injection"] < out["xcor.svd_basis and the subtraction on the host"]
