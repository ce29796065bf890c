"""Detrending the observed exposures on the device, with model injection (trx_detrend_observed, include/transit_hip.h),
against transit_amd.xcor's mirrors of the same definition -- inject_reference, sysrem_reference and, for what the call
installs, weighted_factor -- BIT FOR BIT.

The case is observed_cases.build_case's: pixel_cases.make("eclipse", 20 000 lines, 6001 bins), the 800 pixels with their two off-grid ones
(b = 0 at every exposure), the segments [1, 63, 64, 65, 200, 0, 7, 400], 7 exposures, and a set of 12 exposures for 9
components.  The data are sysrem_cases.data_set (smooth trends plus seeded noise) at the model's scale; the edge weights are
sysrem_cases.edge_weights: 5 % single masked entries, a column masked at every exposure and an exposure masked over a whole
segment.  The exposure and the order axis -- 64, 65 and 130 exposures with up to 16 components, 64, 65 and 130 segments --
are test_gpu_many_exposures.py's.

One refusal of the header's list cannot be reached on a device -- nexp * npix above what one pixel launch takes needs more
than 5e11 pairs --; tests/sysrem_check.cpp holds its text on the host."""
import ctypes as C
import time

import numpy as np
import pytest

import observed_cases as oc
import pixel_cases as pc
import sysrem_cases as sc
import xcor_checks as xc
from bits import same_bits
from transit_amd import _abi, bands, broaden, pixels, xcor
from transit_amd.engine import Engine, EngineError
from transit_amd.exposures import Exposures

pytestmark = pytest.mark.gpu

SHIFTS = pc.SHIFTS


class Case(oc.SysremCase):
    def mirror(self, nexp, weighted, ncomp, niter):
        """xcor.sysrem_reference of the raw set, made once"""
        ob = self.observed(nexp, weighted)
        return self.memo((nexp, weighted, ncomp, niter), lambda: xcor.sysrem_reference(ob.data, ob.weight, ob.seg_first, ncomp, niter))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return oc.build_case(tmp_path_factory.mktemp("sysrem"), Case)


# ---- 1. bits without injection --------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nexp,ncomp", [(7, 1), (7, 3), (7, 5), (12, 9)])
def test_bits_without_injection(case, nexp, ncomp, weighted):
    ob = case.observed(nexp, weighted)
    E = case.handle(ob)
    for niter in (1, 10):
        what = "nexp %d, ncomp %d, niter %d, %s" % (nexp, ncomp, niter, "edge weights" if weighted else "no weights")
        D = E.detrend_observed(ncomp, niter)
        mirror = case.mirror(nexp, weighted, ncomp, niter)
        oc.check_sysrem_outputs(D, mirror, ob, what)
        assert D.spectrum is None
        basis, coef, resid = mirror
        # the edges: the empty segment's vectors are zero, every other segment has a first component
        assert np.all(basis[5] == 0) and np.all(np.any(basis[[0, 1, 2, 3, 4, 6, 7], :, 0] != 0, axis=1)), what
        if weighted:
            k = slice(sc.SEG[sc.MASKED_SEG], sc.SEG[sc.MASKED_SEG + 1])
            assert np.all(D.basis[sc.MASKED_SEG, sc.MASKED_EXP] == 0) and not np.signbit(D.basis[sc.MASKED_SEG, sc.MASKED_EXP]).any(), what
            assert np.array_equal(D.data[sc.MASKED_EXP, k], ob.data[sc.MASKED_EXP, k]), what
            assert np.all(D.coef[:, sc.MASKED_COL] == 0) and np.array_equal(D.data[:, sc.MASKED_COL], ob.data[:, sc.MASKED_COL]), what
            assert D.nsingular >= 1, what                    # (the masked column at the least)
        print("%s: basis, coef, data and nsingular (%d) are the mirror's" % (what, D.nsingular))
    E.close()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nexp", [8, 9, 16, 17])
def test_bits_about_a_whole_number_of_trips(case, nexp, weighted):
    """the column kernels take 8 exposures a trip (kSysTrips): one and two whole trips, and one exposure past each"""
    ob = case.observed(nexp, weighted)
    E = case.handle(ob)
    oc.check_sysrem_outputs(E.detrend_observed(2, 2), case.mirror(nexp, weighted, 2, 2), ob, "%d exposures, %s" % (nexp, "edge weights" if weighted else "no weights"))
    E.close()


# ---- 2. bits with injection -----------------------------------------------------------------------------------
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
    if setup != "pixels":
        assert not np.array_equal(pairs, E.run_pixels(P.atm, P.opts, SHIFTS))
    p0, p1 = 0.05 / case.scale, 0.9
    f0 = xcor.inject_reference(pairs, ob, p0, p1)
    on = pairs[..., 1] > 0
    for p in xc.OFF_GRID:                                    # the off-grid pixels keep F
        assert not on[:, p].any() and same_bits(f0[:, p], ob.data[:, p])
    assert np.count_nonzero(on) > 7 * 700 and np.all(f0[on] != ob.data[on])
    mirror = xcor.sysrem_reference(f0, ob.weight, ob.seg_first, 3, 10)
    D = E.detrend_observed(3, 10, inject=(P.atm, P.opts, SHIFTS, p0, p1))
    oc.check_sysrem_outputs(D, mirror, ob, setup)
    assert np.array_equal(D.spectrum, case.spec)             # run()'s bits, never the broadened spectrum
    assert not same_bits(D.data, case.mirror(7, True, 3, 10)[2])
    # p0 = 0, p1 = 1 injects nothing
    D0 = E.detrend_observed(3, 10, inject=(P.atm, P.opts, SHIFTS, 0.0, 1.0))
    oc.check_sysrem_outputs(D0, case.mirror(7, True, 3, 10), ob, setup + ", p0 = 0 and p1 = 1")
    E.close()


# ---- 3. from raw, always; the undo ----------------------------------------------------------------------------
def test_from_raw_and_the_undo(case):
    P = case.P
    ob = case.observed(7, True)
    E = case.handle(ob)
    fresh = E.run_moments(P.atm, P.opts, SHIFTS)
    undo = E.detrend_observed(0)                             # nothing had been detrended: TRX_OK
    assert undo.data is None and undo.nsingular == 0 and same_bits(E.run_moments(P.atm, P.opts, SHIFTS), fresh)
    D1 = E.detrend_observed(3, 10)
    oc.check_sysrem_outputs(D1, case.mirror(7, True, 3, 10), ob, "first call")
    assert not same_bits(E.run_moments(P.atm, P.opts, SHIFTS), fresh)
    assert oc.same_detrend(E.detrend_observed(3, 10), D1)        # two identical calls
    inject = (P.atm, P.opts, SHIFTS, 0.05 / case.scale, 1.0)
    other = E.detrend_observed(5, 2, inject=inject)
    assert other.basis.shape == (8, 7, 5) and not same_bits(other.data, D1.data)
    assert oc.same_detrend(E.detrend_observed(3, 10), D1)        # after a different call: a fresh handle's call
    assert oc.same_detrend(E.detrend_observed(5, 2, inject=inject), other)
    quiet = E.detrend_observed(3, 10, outputs=False)
    assert quiet.basis is None and quiet.data is None and quiet.nsingular == D1.nsingular
    mom = E.run_filtered_moments(P.atm, P.opts, SHIFTS)
    # the undo: the raw data back, the filter slot cleared
    undo = E.detrend_observed(0)
    assert undo.nsingular == 0
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), fresh)
    with pytest.raises(EngineError) as ei:
        E.run_filtered_moments(P.atm, P.opts, SHIFTS)
    assert ei.value.code == -1 and "no filter installed" in str(ei.value)
    assert E.detrend_observed(0).nsingular == 0              # twice
    assert oc.same_detrend(E.detrend_observed(3, 10), D1)
    assert same_bits(E.run_filtered_moments(P.atm, P.opts, SHIFTS), mom)
    # the undo also clears a filter the caller installed; set_observed drops the raw copy with the set
    E.detrend_observed(0)
    E.set_filter(xcor.svd_filter(ob.data, ob.seg_first, 2))
    E.detrend_observed(0)
    with pytest.raises(EngineError):
        E.run_filtered_moments(P.atm, P.opts, SHIFTS)
    E.detrend_observed(3, 10)
    ob12 = case.observed(12, True)
    E.set_observed(ob12)
    oc.check_sysrem_outputs(E.detrend_observed(9, 1), case.mirror(12, True, 9, 1), ob12, "after set_observed")
    E.close()


# ---- 4. what is installed --------------------------------------------------------------------------------------
def test_what_is_installed(case):
    P = case.P
    ob = case.observed(7, True)
    hp, ex, vm = xcor.gaussian_highpass(6.0), Exposures(xc.SCALE0.copy(), xc.SMEAR.copy()), xc.the_filtered_map("ccf", offset=True)
    E = case.handle(ob)
    E.set_filter(xcor.svd_filter(ob.data, ob.seg_first, 2))  # a plain filter in the slot: replaced
    E.set_highpass(hp)
    E.set_exposures(ex)
    E.set_broadening(broaden.Rotation(4.0, 0.4))
    exposed, highpassed = E.run_exposed(P.atm, P.opts, SHIFTS), E.run_highpassed(P.atm, P.opts, SHIFTS)
    D = E.detrend_observed(3, 10)
    basis, coef, resid = case.mirror(7, True, 3, 10)
    oc.check_sysrem_outputs(D, (basis, coef, resid), ob, "behind a high-pass, a table and a broadening")
    got = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    got_map = E.run_exposed_map(P.atm, P.opts, vm)
    F = case.handle(xcor.Observed(ob.seg_first, resid, ob.weight, ob.gain))
    assert F.set_weighted_filter(xcor.WeightedFilter(basis)) == D.nsingular
    F.set_highpass(hp)
    F.set_exposures(ex)
    F.set_broadening(broaden.Rotation(4.0, 0.4))
    want = F.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    want_map = F.run_exposed_map(P.atm, P.opts, vm)
    F.close()
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert same_bits(got_map, want_map) and np.array_equal(np.isnan(got_map), xc.OUTSIDE)
    assert np.count_nonzero(np.isfinite(got[1]).all(axis=0)) > 700 and np.isnan(got[1][:, sc.MASKED_COL]).all()
    # the high-pass, the table and the broadening survive the call
    assert same_bits(E.run_exposed(P.atm, P.opts, SHIFTS), exposed) and same_bits(E.run_highpassed(P.atm, P.opts, SHIFTS), highpassed)
    E.close()


# ---- 5. no trace; refusals --------------------------------------------------------------------------------------
def test_no_trace_and_refusals(case):
    P = case.P
    ob = case.observed(7, True)
    E = case.handle(ob)
    E.set_bands([bands.gauss(2520.0, 0.5), bands.gauss(2540.0, 2.0)])
    p0 = 0.05 / case.scale

    def neighbours():
        return [E.run(P.atm, P.opts)["spectrum"], E.run_pixels(P.atm, P.opts, SHIFTS), E.run_bands(P.atm, P.opts)]

    before = neighbours()
    assert np.array_equal(before[0], case.spec)
    D = E.detrend_observed(3, 10, inject=(P.atm, P.opts, SHIFTS, p0, 1.0))
    assert all(same_bits(a, b) for a, b in zip(neighbours(), before))
    E.detrend_observed(3, 10)
    assert all(same_bits(a, b) for a, b in zip(neighbours(), before))
    E.detrend_observed(3, 10, inject=(P.atm, P.opts, SHIFTS, p0, 1.0))
    ref = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)

    lib, dp = E._lib, _abi.c_double_p
    basis, coef, data = np.full((8, 7, 3), -7.0), np.full((3, 800), -7.0), np.full((7, 800), -7.0)
    spec, ns = np.full(P.nwn, -7.0), C.c_int64(-7)
    bad_shift = SHIFTS.copy()
    bad_shift[4] = -1.0

    def raw(dt, a=P.atm, o=P.opts, nshift=7, shift=SHIFTS):
        rc = lib.trx_detrend_observed(E._h, C.byref(a) if a is not None else None, C.byref(o) if o is not None else None, spec.ctypes.data_as(dp),
                                      nshift, shift.ctypes.data_as(dp) if shift is not None else None, C.byref(dt), basis.ctypes.data_as(dp),
                                      coef.ctypes.data_as(dp), data.ctypes.data_as(dp), C.byref(ns), None)
        # a refusal touches no output
        assert np.all(basis == -7.0) and np.all(coef == -7.0) and np.all(data == -7.0) and np.all(spec == -7.0) and ns.value == -7
        return rc, E._last_error()

    def dt(**fields):
        d = _abi.TrxDetrend(3, 10, 1, 0, p0, 1.0)
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    who = "trx_detrend_observed: "
    assert raw(dt(ncomp=-1)) == (-1, who + "ncomp < 0")
    assert raw(dt(ncomp=17)) == (-1, who + "ncomp above TRX_FILTER_MAX (16)")
    assert raw(dt(niter=0)) == (-1, who + "niter < 1")
    assert raw(dt(niter=65)) == (-1, who + "niter above TRX_SYSREM_MAX_ITER (64)")
    assert raw(dt(inject=2)) == (-1, who + "inject must be 0 or 1")
    assert raw(dt(pad=1)) == (-1, who + "pad must be 0")
    assert raw(dt(p0=float("nan"))) == (-1, who + "p0 must be finite")
    assert raw(dt(p1=float("inf"))) == (-1, who + "p1 must be finite")
    assert raw(dt(), a=None) == (-1, who + "a is NULL")
    assert raw(dt(), o=None) == (-1, who + "o is NULL")
    assert raw(dt(), shift=None) == (-1, who + "shift is NULL")
    assert raw(dt(), nshift=6) == (-1, who + "nshift 6 is not the observed set's nexp 7")
    assert raw(dt(), shift=bad_shift) == (-1, who + "shift 4 must be finite and > 0")
    # the order: the first fault in the header's list is the one named
    assert raw(dt(ncomp=17, niter=0, inject=2, pad=1), a=None) == (-1, who + "ncomp above TRX_FILTER_MAX (16)")
    assert raw(dt(niter=65, pad=1, p0=float("nan")), shift=None) == (-1, who + "niter above TRX_SYSREM_MAX_ITER (64)")
    # after the refusals: the data and the filter of the last good call
    after = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    assert same_bits(after[0], ref[0]) and same_bits(after[1], ref[1])
    assert oc.same_detrend(E.detrend_observed(3, 10, inject=(P.atm, P.opts, SHIFTS, p0, 1.0)), D)
    E.close()
    # no observed set
    N = case.handle(None)
    for ncomp in (3, 0):
        with pytest.raises(EngineError) as ei:
            N.detrend_observed(ncomp)
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
                S.detrend_observed(1, 2, inject=inject)
            assert ei.value.code == -6 and who + "this handle's shard is not the whole grid" in str(ei.value)
        assert S.run_pixels(P.atm, P.opts, SHIFTS).shape == (7, 4, 2)
        S.close()
    finally:
        P.set_shard(0, n)


# ---- 6. injection and recovery, end to end -----------------------------------------------------------------------
def test_injection_and_recovery_end_to_end(case):
    """Raw data: a continuum with smooth trends in time plus seeded noise, two segments (the pixels at R = 20 000 and those at
    R = 3000).  The model is injected with p1 = 1 at the cell (Kp, Vsys) = (100, 6) km/s of test_gpu_trail's 5 x 5 map,
    SYSREM takes two components, and the CCF map of trx_run_exposed_map is the recovery."""
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
    # the precondition, on the host from the device's pairs: the numpy chain alone finds the injected cell, and does not
    # without the injection
    injected = E.run_exposed(P.atm, P.opts, shifts)
    pairs_lv = np.stack([E.run_exposed(P.atm, P.opts, np.full(7, s)) for s in xc.LAGS])

    def host_map(data):
        basis, coef, resid = xcor.sysrem_reference(data, w, seg, 2, 10)
        return xcor.exposed_map_reference(pairs_lv, xcor.Observed(seg, resid, w, ob.gain), xcor.WeightedFilter(basis), vm)

    def peak(m):
        assert np.isfinite(m).all()
        return tuple(int(i) for i in np.unravel_index(np.argmax(m), m.shape))

    with_injection, without = host_map(xcor.inject_reference(injected, ob, p0, 1.0)), host_map(raw)
    print("numpy chain, injected (rows Kp, columns Vsys):\n%s\nnumpy chain, not injected:\n%s"
          % (np.array2string(with_injection, precision=4), np.array2string(without, precision=4)))
    assert peak(with_injection) == cell and peak(without) != cell
    # the device
    E.detrend_observed(2, 10, inject=(P.atm, P.opts, shifts, p0, 1.0), outputs=False)
    m, idx = E.run_exposed_map(P.atm, P.opts, vm, lag_index=True)
    print("device:\n%s" % np.array2string(m, precision=4))
    assert np.array_equal(idx, xcor.nearest_lags(vm)) and np.all(idx >= 0)
    assert peak(m) == cell
    # every cell keeps trx_run_exposed_map's contract against run_filtered_moments on the same handle
    differ = 0
    for i in range(5):
        for j in range(5):
            mom = E.run_filtered_moments(P.atm, P.opts, xc.LAGS[idx[i, j]])
            want, bound = xcor.cell_value(mom, vm), xcor.cell_bound(mom, vm)
            assert bound > 0 and abs(m[i, j] - want) <= bound, (i, j, m[i, j], want, bound)
            differ += m[i, j] != want
    print("%d of 25 cells differ in bits from cell_value(run_filtered_moments); worst |device - numpy chain| %.3e"
          % (differ, float(np.max(np.abs(m - with_injection)))))
    E.close()


# ---- 7. size and time --------------------------------------------------------------------------------------------
def test_size_and_time(case):
    """40 orders of 2048 pixels, 100 exposures, 5 components of 10 alternations: determinism and finiteness are asserted,
    the times are printed (a host clock around calls that return synchronised, after one warm-up call, the mean of 20)."""
    P = case.P
    nseg, n, nexp, ncomp, niter, reps = 40, 2048, 100, 5, 10, 20
    npix = nseg * n
    px = pixels.resolving_power(np.linspace(2503.0, 2557.0, npix), 20000.0, 4.0)
    rng = np.random.default_rng(5)
    seg = xcor.segments([n] * nseg)
    x, t = np.linspace(0.0, 1.0, npix), np.linspace(-1.0, 1.0, nexp)
    raw = (1.0 + 0.3 * np.sin(40.0 * x))[None, :] * (1.0 + 0.05 * t[:, None] * np.sin(9.0 * x)[None, :] + 0.02 * (t ** 2)[:, None])
    raw = case.scale * (raw + 1e-3 * rng.standard_normal((nexp, npix)))
    w = rng.uniform(0.5, 2.0, (nexp, npix))
    w[rng.random((nexp, npix)) < 0.02] = 0.0
    ob = xcor.Observed(seg, raw, w)
    shifts = np.array([pixels.shift(v) for v in np.linspace(-40.0, 40.0, nexp)])
    E = Engine(P.static)
    E.set_pixels(px)
    E.set_observed(ob)
    out = {}
    for name, inject in (("without injection", None), ("with injection", (P.atm, P.opts, shifts, 0.05 / case.scale, 1.0))):
        first = E.detrend_observed(ncomp, niter, inject=inject)              # (the warm-up)
        t0 = time.perf_counter()
        for _ in range(reps):
            E.detrend_observed(ncomp, niter, inject=inject, outputs=False)
        out[name] = (time.perf_counter() - t0) / reps
        t0 = time.perf_counter()
        again = E.detrend_observed(ncomp, niter, inject=inject)
        out[name + ", outputs copied"] = time.perf_counter() - t0
        assert oc.same_detrend(first, again), name
        assert np.isfinite(first.basis).all() and np.isfinite(first.coef).all() and np.isfinite(first.data).all(), name
        assert first.basis.shape == (nseg, nexp, ncomp) and np.all(np.abs(np.linalg.norm(first.basis, axis=1) - 1.0) < 1e-12), name
    t0 = time.perf_counter()
    host = xcor.sysrem_basis(raw, w, seg, 1, niter=niter)
    out["xcor.sysrem_basis on the host, one component"] = time.perf_counter() - t0
    assert np.isfinite(host).all()
    E.close()
    print("40 x 2048 pixels, 100 exposures, %d components of %d alternations:" % (ncomp, niter))
    for name, s in out.items():
        print("  %-50s %9.3f ms" % (name, 1e3 * s))
