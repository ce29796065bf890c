"""Weighing the observed set by its columns' scatter on the device (trx_weigh_observed, include/transit_hip.h) against
transit_amd.xcor.scatter_reference, the numpy mirror of the same definition -- BIT FOR BIT --, and, for what the call
leaves installed, against a fresh handle that gets the same data, weights and basis through set_observed and
set_weighted_filter.

The case is observed_cases.build_case's: pixel_cases.make("eclipse", 20 000 lines, 6001 bins), the 800 pixels, the segments [1, 63, 64, 65,
200, 0, 7, 400], 7 and 12 exposures.  The data are scatter_cases.the_set at the model's scale: faint trends plus seeded
noise with the planted columns (the ties at the median rank of the 65- and the 200-pixel segment, a constant column, a
column masked at every exposure, five columns of 10 x the noise); tests/test_scatter_host.py holds their preconditions."""
import ctypes as C
import time

import numpy as np
import pytest

import observed_cases as oc
import pixel_cases as pc
import scatter_cases as cs
import xcor_checks as xc
from bits import same_bits
from transit_amd import _abi, pixels, xcor
from transit_amd.engine import Engine, EngineError
from transit_amd.exposures import Exposures

pytestmark = pytest.mark.gpu

SHIFTS = pc.SHIFTS
V, M = xcor.SCATTER_VARIANCE, xcor.SCATTER_MASK


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return oc.build_case(tmp_path_factory.mktemp("scatter"), oc.ScatterCase)


def same_result(a, b):
    return same_bits(a.variance, b.variance) and same_bits(a.median, b.median) and same_bits(a.weight, b.weight) and \
        (a.nmasked, a.nsingular) == (b.nmasked, b.nsingular)


# ---- 1. the outputs' bits, on the raw data and on the residuals of a detrend ---------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nexp", [7, 12])
def test_bits(case, nexp, weighted):
    ob = case.observed(nexp, weighted)
    E = case.handle(ob)
    for stage in ("raw", "detrended"):
        D = E.detrend_observed(3, niter=2) if stage == "detrended" else None
        data = D.data if D else ob.data
        for kind in cs.KINDS:
            for clip in cs.CLIPS:
                for min_live in (2, nexp):
                    what = "nexp %d, %s, %s, kind %d, clip %g, min_live %d" % (nexp, "edge weights" if weighted else "no weights", stage, kind, clip, min_live)
                    mirror = xcor.scatter_reference(data, ob.weight, ob.seg_first, kind, clip, min_live)
                    R = E.weigh_observed(kind, clip=clip, min_live=min_live)
                    oc.check_scatter_outputs(R, mirror, what)
                    assert R.nsingular == (oc.nsingular_of(ob, D.basis, data, mirror[3]) if D else 0), what
                    if clip:
                        clipped, margin = cs.clip_margin(*mirror[:3])
                        print("%s: clipped %s, nearest var / (9 med) %.3f away from 1, nsingular %d" % (what, clipped, margin, R.nsingular))
                        assert margin > 0.05, what
                        if stage == "raw":
                            assert clipped == tuple(p for p in cs.NOISY_COLS if mirror[0][p] > 0), what
    E.close()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nexp", [8, 9, 16, 17])
def test_bits_about_a_whole_number_of_trips(case, nexp, weighted):
    """the column kernels take 8 exposures a trip (kSysTrips): one and two whole trips, and one exposure past each"""
    ob = case.observed(nexp, weighted)
    E = case.handle(ob)
    mirror = xcor.scatter_reference(ob.data, ob.weight, ob.seg_first, V, 3.0, 2)
    assert np.isfinite(mirror[0]).all() and np.isfinite(mirror[3]).all()
    oc.check_scatter_outputs(E.weigh_observed(V, clip=3.0, min_live=2), mirror, "%d exposures, %s" % (nexp, "edge weights" if weighted else "no weights"))
    E.close()


# ---- 2. what is installed ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cs.KINDS)
def test_what_is_installed(case, kind):
    P = case.P
    ob = case.observed(7, True)
    E = case.handle(ob)
    D = E.detrend_observed(3, niter=2)
    R = E.weigh_observed(kind, clip=3.0)
    assert R.nmasked == 5
    got = (E.run_moments(P.atm, P.opts, SHIFTS),) + tuple(E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True))
    F = case.handle(xcor.Observed(ob.seg_first, D.data, R.weight, ob.gain))
    assert F.set_weighted_filter(xcor.WeightedFilter(D.basis)) == R.nsingular
    want = (F.run_moments(P.atm, P.opts, SHIFTS),) + tuple(F.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True))
    assert all(same_bits(a, b) for a, b in zip(got, want))
    assert np.isnan(got[2][:, list(cs.NOISY_COLS)]).all() and np.count_nonzero(np.isfinite(got[2]).all(axis=0)) > 700
    # a weighted filter installed after the weigh is factorised against the weights in force
    assert E.set_weighted_filter(xcor.WeightedFilter(D.basis)) == R.nsingular
    again = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    assert same_bits(again[0], want[1]) and same_bits(again[1], want[2])
    # a weighted filter the caller installed over the raw set is factorised again by the weigh
    E.detrend_observed(0)
    E.set_weighted_filter(xcor.WeightedFilter(D.basis))
    R0 = E.weigh_observed(kind, clip=3.0)
    got0 = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    F.set_observed(xcor.Observed(ob.seg_first, ob.data, R0.weight, ob.gain))
    assert F.set_weighted_filter(xcor.WeightedFilter(D.basis)) == R0.nsingular
    want0 = F.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    assert same_bits(got0[0], want0[0]) and same_bits(got0[1], want0[1])
    assert not same_bits(R0.weight, R.weight)
    F.close()
    E.close()


# ---- 3. from raw, always; the undo ----------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [True, False])
def test_from_raw_and_the_undo(case, weighted):
    P = case.P
    ob = case.observed(7, weighted)
    E = case.handle(ob)
    raw_mom = E.run_moments(P.atm, P.opts, SHIFTS)
    undo = E.weigh_observed(xcor.SCATTER_NONE)               # nothing had been weighed: TRX_OK
    assert undo.weight is None and (undo.nmasked, undo.nsingular) == (0, 0) and same_bits(E.run_moments(P.atm, P.opts, SHIFTS), raw_mom)
    D1 = E.detrend_observed(3, niter=2)
    mom, fmom = E.run_moments(P.atm, P.opts, SHIFTS), E.run_filtered_moments(P.atm, P.opts, SHIFTS)
    R1 = E.weigh_observed(V, clip=3.0)
    oc.check_scatter_outputs(R1, xcor.scatter_reference(D1.data, ob.weight, ob.seg_first, V, 3.0, 2), "first call")
    wmom, wfmom = E.run_moments(P.atm, P.opts, SHIFTS), E.run_filtered_moments(P.atm, P.opts, SHIFTS)
    assert not same_bits(wmom, mom) and not same_bits(wfmom, fmom)
    assert same_result(E.weigh_observed(V, clip=3.0), R1)    # twice: W is never an earlier call's result
    other = E.weigh_observed(M, clip=0.0, min_live=7)
    assert not same_bits(other.weight, R1.weight)
    assert same_result(E.weigh_observed(V, clip=3.0), R1)    # after a different call
    quiet = E.weigh_observed(V, clip=3.0, outputs=False)
    assert quiet.weight is None and quiet.variance is None and (quiet.nmasked, quiet.nsingular) == (R1.nmasked, R1.nsingular)
    assert same_bits(E.run_filtered_moments(P.atm, P.opts, SHIFTS), wfmom)
    # the undo: the moments from before the weigh
    undo = E.weigh_observed(xcor.SCATTER_NONE)
    assert undo.nsingular == D1.nsingular and undo.nmasked == 0
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), mom) and same_bits(E.run_filtered_moments(P.atm, P.opts, SHIFTS), fmom)
    assert E.weigh_observed(xcor.SCATTER_NONE).nsingular == D1.nsingular      # twice
    assert same_bits(E.run_filtered_moments(P.atm, P.opts, SHIFTS), fmom)
    # detrend, weigh, detrend: the second detrend is a fresh handle's single one, and so is what follows it
    assert same_result(E.weigh_observed(V, clip=3.0), R1)
    D2 = E.detrend_observed(3, niter=2)
    F = case.handle(ob)
    DF = F.detrend_observed(3, niter=2)
    assert oc.same_detrend(D2, DF) and oc.same_detrend(D2, D1)
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), F.run_moments(P.atm, P.opts, SHIFTS))
    assert same_bits(E.run_filtered_moments(P.atm, P.opts, SHIFTS), F.run_filtered_moments(P.atm, P.opts, SHIFTS))
    assert same_bits(E.run_filtered_moments(P.atm, P.opts, SHIFTS), fmom)
    F.close()
    # the detrend's own undo after a weigh: the raw data AND the weights of set_observed
    E.weigh_observed(M, clip=3.0)
    E.detrend_observed(0)
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), raw_mom)
    # set_observed drops everything
    E.weigh_observed(V, clip=3.0)
    ob12 = case.observed(12, weighted)
    E.set_observed(ob12)
    oc.check_scatter_outputs(E.weigh_observed(M, clip=3.0, min_live=12), xcor.scatter_reference(ob12.data, ob12.weight, ob12.seg_first, M, 3.0, 12), "after set_observed")
    E.close()


# ---- 4. a plain filter survives ---------------------------------------------------------------------------------
def test_a_plain_filter_survives(case):
    P = case.P
    ob = case.observed(7, True)
    filt = xcor.svd_filter(ob.data, ob.seg_first, 2)
    E = case.handle(ob)
    E.set_filter(filt)
    before = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    R = E.weigh_observed(V, clip=3.0)
    assert R.nsingular == 0 and R.nmasked == 5
    got = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    assert same_bits(got[1], before[1]) and not same_bits(got[0], before[0])      # the plain filter's values know no weights
    F = case.handle(xcor.Observed(ob.seg_first, ob.data, R.weight, ob.gain))
    F.set_filter(filt)
    want = F.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    F.close()
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert E.weigh_observed(xcor.SCATTER_NONE).nsingular == 0
    after = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    assert same_bits(after[0], before[0]) and same_bits(after[1], before[1])
    E.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(case):
    P = case.P
    ob = case.observed(7, True)
    E = case.handle(ob)
    E.detrend_observed(3, niter=2)
    good = E.weigh_observed(V, clip=3.0)
    ref = (E.run_moments(P.atm, P.opts, SHIFTS),) + tuple(E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True))
    lib, dp = E._lib, _abi.c_double_p
    var, med, w = np.full(800, -7.0), np.full(8, -7.0), np.full((7, 800), -7.0)
    nm, ns = C.c_int64(-7), C.c_int64(-7)

    def raw(kind=V, min_live=2, clip=3.0):
        sc = _abi.TrxScatter(kind, min_live, clip)
        rc = lib.trx_weigh_observed(E._h, C.byref(sc), var.ctypes.data_as(dp), med.ctypes.data_as(dp), w.ctypes.data_as(dp), C.byref(nm), C.byref(ns))
        # a refusal touches no output
        assert np.all(var == -7.0) and np.all(med == -7.0) and np.all(w == -7.0) and (nm.value, ns.value) == (-7, -7)
        return rc, E._last_error()

    who = "trx_weigh_observed: "
    assert raw(kind=3) == (-1, who + "kind must be TRX_SCATTER_NONE, _VARIANCE or _MASK")
    assert raw(kind=-1) == (-1, who + "kind must be TRX_SCATTER_NONE, _VARIANCE or _MASK")
    assert raw(min_live=1) == (-1, who + "min_live < 2")
    assert raw(min_live=8) == (-1, who + "min_live 8 is above the observed set's nexp 7")
    assert raw(clip=float("nan")) == (-1, who + "clip must be finite")
    assert raw(clip=float("inf")) == (-1, who + "clip must be finite")
    assert raw(clip=-3.0) == (-1, who + "clip < 0")
    assert raw(clip=0.5) == (-1, who + "clip must be 0 (none) or at least 1")
    # the order: the first fault in the header's list is the one named
    assert raw(kind=7, min_live=0, clip=float("nan")) == (-1, who + "kind must be TRX_SCATTER_NONE, _VARIANCE or _MASK")
    assert raw(min_live=9, clip=-1.0) == (-1, who + "min_live 9 is above the observed set's nexp 7")
    assert raw(kind=xcor.SCATTER_NONE, min_live=1) == (-1, who + "min_live < 2")
    # after the refusals: the weights and the filter of the last good call
    after = (E.run_moments(P.atm, P.opts, SHIFTS),) + tuple(E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True))
    assert all(same_bits(a, b) for a, b in zip(after, ref))
    assert same_result(E.weigh_observed(V, clip=3.0), good)
    E.close()
    # no observed set
    N = case.handle(None)
    for kind in (V, xcor.SCATTER_NONE):
        with pytest.raises(EngineError) as ei:
            N.weigh_observed(kind)
        assert ei.value.code == -1 and who + "no observed set installed (trx_set_observed)" in str(ei.value)
    N.close()
    # a shard of the grid
    n = P.nwn
    try:
        P.set_shard(1000, 3000)
        S = Engine(P.static)
        S.set_pixels(pixels.Pixels([2510.0, 2520.0, 2530.0, 2540.0], [0.2, 0.3, 1.5, 0.4], 4.0))
        S.set_observed(xcor.Observed([0, 1, 4], np.ones((7, 4))))
        for kind in (V, xcor.SCATTER_NONE):
            with pytest.raises(EngineError) as ei:
                S.weigh_observed(kind)
            assert ei.value.code == -6 and who + "this handle's shard is not the whole grid" in str(ei.value)
        S.close()
    finally:
        P.set_shard(0, n)


# ---- 6. injection, detrend, weigh and recovery, end to end --------------------------------------------------------
def test_injection_weights_and_recovery_end_to_end(case):
    """test_gpu_sysrem's end-to-end set -- a continuum with smooth trends in time plus seeded noise, two segments -- with five
    columns of 10 x the noise.  The model is injected at the cell (Kp, Vsys) = (100, 6) km/s of test_gpu_trail's 5 x 5 map,
    SYSREM takes two components, the columns are weighed by their inverse variance with a clip of 3, and the CCF map of
    trx_run_exposed_map is the recovery."""
    P = case.P
    rng = np.random.default_rng(21)
    seg = xcor.segments([400, 400])
    x, t = np.linspace(0.0, 1.0, 800), np.linspace(-1.0, 1.0, 7)
    trend = (1.0 + 0.3 * np.sin(5.0 * x))[None, :] * (1.0 + 0.1 * t[:, None] + 0.05 * (t ** 2)[:, None] * np.cos(3.0 * x)[None, :])
    noise = 1e-4 * rng.standard_normal((7, 800))
    noisy = (37, 300, 411, 640, 777)
    noise[:, noisy] *= 10.0
    raw = case.scale * (trend + noise)
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

    def peak(m):
        assert np.isfinite(m).all()
        return tuple(int(i) for i in np.unravel_index(np.argmax(m), m.shape))

    # the precondition, on the host from the device's pairs: the numpy chain alone -- inject, SYSREM, weigh, map -- finds the
    # injected cell, and does not without the injection
    injected = E.run_exposed(P.atm, P.opts, shifts)
    pairs_lv = np.stack([E.run_exposed(P.atm, P.opts, np.full(7, s)) for s in xc.LAGS])

    def host_map(data):
        basis, coef, resid = xcor.sysrem_reference(data, w, seg, 2, 10)
        var, med, keep, w1 = xcor.scatter_reference(resid, w, seg, V, 3.0, 2)
        return xcor.exposed_map_reference(pairs_lv, xcor.Observed(seg, resid, w1, ob.gain), xcor.WeightedFilter(basis), vm), (var, med, keep, w1)

    (with_injection, mirror), (without, _) = host_map(xcor.inject_reference(injected, ob, p0, 1.0)), host_map(raw)
    print("numpy chain, injected (rows Kp, columns Vsys):\n%s\nnumpy chain, not injected:\n%s"
          % (np.array2string(with_injection, precision=4), np.array2string(without, precision=4)))
    assert peak(with_injection) == cell and peak(without) != cell
    # the device
    E.detrend_observed(2, 10, inject=(P.atm, P.opts, shifts, p0, 1.0), outputs=False)
    R = E.weigh_observed(V, clip=3.0)
    oc.check_scatter_outputs(R, mirror, "end to end")
    print("%d columns clipped (%s of the five noisy ones among them), %d dead in the filter"
          % (R.nmasked, sum(R.weight[:, p].max() == 0 for p in noisy), R.nsingular))
    assert 5 <= R.nmasked < 400
    m, idx = E.run_exposed_map(P.atm, P.opts, vm, lag_index=True)
    print("device (rows Kp, columns Vsys):\n%s" % np.array2string(m, precision=4))
    assert np.array_equal(idx, xcor.nearest_lags(vm)) and np.all(idx >= 0)
    assert peak(m) == cell
    # every cell has the bits of the same handle's filtered moments at the cell's lags
    for i in range(5):
        for j in range(5):
            mom = E.run_filtered_moments(P.atm, P.opts, xc.LAGS[idx[i, j]])
            want = xcor.cell_value(mom, vm)
            assert same_bits(m[i, j], want), (i, j, m[i, j], want)
    E.close()


# ---- 7. size and time --------------------------------------------------------------------------------------------
def test_size_and_time(case):
    """40 orders of 2048 pixels, 100 exposures, a warm handle: the device call with its outputs left on the device (a host
    clock around calls that return synchronised, after one warm-up call, the mean of 20) must be faster than
    xcor.scatter_reference on the host, measured here; a streaming pass that loses to numpy means a mis-sized launch or a
    quadratic median.  detrend_observed(5, 10) alone is printed for scale."""
    P = case.P
    nseg, n, nexp, reps = 40, 2048, 100, 20
    npix = nseg * n
    px = pixels.resolving_power(np.linspace(2503.0, 2557.0, npix), 20000.0, 4.0)
    rng = np.random.default_rng(5)
    seg = xcor.segments([n] * nseg)
    x, t = np.linspace(0.0, 1.0, npix), np.linspace(-1.0, 1.0, nexp)
    raw = (1.0 + 0.3 * np.sin(40.0 * x))[None, :] * (1.0 + 0.05 * t[:, None] * np.sin(9.0 * x)[None, :] + 0.02 * (t ** 2)[:, None])
    raw = case.scale * (raw + 1e-3 * rng.standard_normal((nexp, npix)))
    w = rng.uniform(0.5, 2.0, (nexp, npix))
    w[rng.random((nexp, npix)) < 0.02] = 0.0
    E = Engine(P.static)
    E.set_pixels(px)
    E.set_observed(xcor.Observed(seg, raw, w))
    D = E.detrend_observed(5, 10)                            # (the warm-up of the detrend, and the residuals to weigh)
    t0 = time.perf_counter()
    for _ in range(reps):
        E.detrend_observed(5, 10, outputs=False)
    t_detrend = (time.perf_counter() - t0) / reps
    first = E.weigh_observed(V, clip=3.0)                    # (the warm-up)
    t0 = time.perf_counter()
    for _ in range(reps):
        E.weigh_observed(V, clip=3.0, outputs=False)
    t_device = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    mirror = xcor.scatter_reference(D.data, w, seg, V, 3.0, 2)
    t_host = time.perf_counter() - t0
    oc.check_scatter_outputs(first, mirror, "40 x 2048")
    assert same_result(E.weigh_observed(V, clip=3.0), first)
    E.close()
    print("40 x 2048 pixels, 100 exposures:")
    print("  %-60s %9.3f ms" % ("weigh_observed on the device, outputs left there", 1e3 * t_device))
    print("  %-60s %9.3f ms" % ("xcor.scatter_reference on the host", 1e3 * t_host))
    print("  %-60s %9.3f ms" % ("detrend_observed(5, 10) alone, for scale", 1e3 * t_detrend))
    print("  nmasked %d, nsingular %d" % (first.nmasked, first.nsingular))
    assert t_device < t_host
