"""High-passing the observed set itself on the device (trx_highpass_observed, include/transit_hip.h) against
transit_amd.xcor.highpass_observed_reference, the numpy mirror of the same definition -- BIT FOR BIT, every entry --, against
the model side's own kernel (run_highpassed), and, for what the call leaves installed, against a fresh handle that gets the
same data, weights, basis and high-pass through set_observed, set_weighted_filter and set_highpass.

The case is observed_cases.build_case's: pixel_cases.make("eclipse", 20 000 lines), the 800 pixels, 7 and 12 exposures, scatter_cases.the_set at
the model's scale -- over two segmentations (hpdata_cases.SEGS: the eight orders, and one segment of 736 pixels over two
tiles of 512 with a ragged second one); tests/test_hpdata_host.py holds their preconditions."""
import ctypes as C
import time

import numpy as np
import pytest

import hpdata_cases as hc
import observed_cases as oc
import pixel_cases as pc
import xcor_checks as xc
from bits import same_bits
from transit_amd import _abi, pixels, xcor
from transit_amd.engine import Engine, EngineError
from transit_amd.exposures import Exposures

pytestmark = pytest.mark.gpu

SHIFTS = pc.SHIFTS
SHIFTS12 = np.concatenate([SHIFTS, SHIFTS[1:6] * (1.0 + 1e-5)])
V = xcor.SCATTER_VARIANCE
HP = hc.tables(70)["gauss"]


class Case(oc.ScatterCase):
    def make_observed(self, nexp, weighted, seg_name="orders"):
        """scatter_cases.the_set cut into the segments of this name"""
        return super().make_observed(nexp, weighted, hc.SEGS[seg_name])


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return oc.build_case(tmp_path_factory.mktemp("hpdata"), Case)


def runs(E, P, shifts=SHIFTS):
    return (E.run_moments(P.atm, P.opts, shifts),) + tuple(E.run_filtered_moments(P.atm, P.opts, shifts, values=True))


def same_runs(a, b):
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


def test_the_tables_are_the_model_sides():
    for half in hc.HALVES:
        for name, hp in xc.highpass_tables(half).items():
            assert same_bits(hp.taps, hc.tables(half)[name].taps)


# ---- 1. the outputs' bits, on the raw data and on the residuals of a detrend ---------------------------------
@pytest.mark.parametrize("seg_name", list(hc.SEGS))
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nexp", [7, 12])
def test_bits(case, nexp, weighted, seg_name):
    ob = case.observed(nexp, weighted, seg_name)
    E = case.handle(ob)
    for stage in hc.STAGES:
        data = E.detrend_observed(3, niter=2).data if stage == "detrended" else ob.data
        for half in hc.HALVES:
            for name, hp in hc.tables(half).items():
                what = "nexp %d, %s, %s, %s, half %d, %s" % (nexp, "edge weights" if weighted else "no weights", seg_name, stage, half, name)
                want, ndead = xcor.highpass_observed_reference(data, ob.weight, ob.seg_first, hp)
                E.set_highpass(hp)
                R = E.highpass_observed()
                assert same_bits(R.data, want), what
                assert R.ndead == ndead and (ndead > 0) == weighted, what
    E.close()


# ---- 2. two kernels, one definition ----------------------------------------------------------------------------
@pytest.mark.parametrize("seg_name", list(hc.SEGS))
@pytest.mark.parametrize("nexp", [7, 12])
def test_two_kernels_one_definition(case, nexp, seg_name):
    """the model's values g = gain (a / b) of run_pixels' pairs installed as DATA, live where b > 0, without a gain: the data
    kernel then gives what the model kernel gives of the pairs themselves"""
    P = case.P
    shifts = SHIFTS if nexp == 7 else SHIFTS12
    ob = case.observed(nexp, True, seg_name)
    M = case.handle(ob)
    pairs = M.run_pixels(P.atm, P.opts, shifts)
    a, b = pairs[..., 0], pairs[..., 1]
    live = b > 0
    assert not live[:, list(xc.OFF_GRID)].any() and np.count_nonzero(live.all(axis=0)) > 700
    with np.errstate(all="ignore"):
        g = np.where(live, ob.gain[None, :] * (a / np.where(live, b, 1.0)), 0.0)
    D = case.handle(xcor.Observed(ob.seg_first, g, live.astype(np.float64), None))
    for half in (5, 70, 450):
        for name, hp in hc.tables(half).items():
            M.set_highpass(hp)
            D.set_highpass(hp)
            model = M.run_highpassed(P.atm, P.opts, shifts)
            assert np.array_equal(np.isnan(model), ~live)
            R = D.highpass_observed()
            assert same_bits(R.data, np.where(live, model, 0.0)), (half, name)
            assert R.ndead == np.count_nonzero(~live)
    M.close()
    D.close()


# ---- 3. what is installed ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_name", list(hc.SEGS))
def test_what_is_installed(case, seg_name):
    P = case.P
    ob = case.observed(7, True, seg_name)
    E = case.handle(ob, hp=HP)
    D = E.detrend_observed(3, niter=2)
    before = runs(E, P)
    R = E.highpass_observed()
    got = runs(E, P)
    assert not same_runs(got, before)
    F = case.handle(xcor.Observed(ob.seg_first, R.data, ob.weight, ob.gain))
    assert F.set_weighted_filter(xcor.WeightedFilter(D.basis)) == D.nsingular
    F.set_highpass(HP)
    assert same_runs(got, runs(F, P))
    # outputs=False installs the same data
    E.detrend_observed(3, niter=2, outputs=False)
    quiet = E.highpass_observed(outputs=False)
    assert quiet.data is None and quiet.ndead == R.ndead
    assert same_runs(got, runs(E, P))
    F.close()
    E.close()


# ---- 4. the state ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [True, False])
def test_from_the_detrends_data_and_the_undo(case, weighted):
    P = case.P
    ob = case.observed(7, weighted)
    E = case.handle(ob, hp=HP)
    raw_runs = E.run_moments(P.atm, P.opts, SHIFTS)
    undo = E.highpass_observed(apply=False)                  # nothing had been high-passed: TRX_OK
    assert undo.data is None and undo.ndead == 0 and same_bits(E.run_moments(P.atm, P.opts, SHIFTS), raw_runs)
    # over the raw set: twice is once, the undo gives the raw set's results back
    R0 = E.highpass_observed()
    assert same_bits(R0.data, xcor.highpass_observed_reference(ob.data, ob.weight, ob.seg_first, HP)[0])
    hp_mom = E.run_moments(P.atm, P.opts, SHIFTS)
    assert not same_bits(hp_mom, raw_runs)
    again = E.highpass_observed()
    assert same_bits(again.data, R0.data) and again.ndead == R0.ndead and same_bits(E.run_moments(P.atm, P.opts, SHIFTS), hp_mom)
    E.highpass_observed(apply=False)
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), raw_runs)
    E.highpass_observed(apply=False)                         # twice
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), raw_runs)
    # high-pass, then the detrend's undo: the raw set
    E.highpass_observed()
    E.detrend_observed(0)
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), raw_runs)
    assert same_bits(E.highpass_observed().data, R0.data)    # (and a high-pass after it reads the raw set)
    # over the residuals: twice is once, the undo gives the residuals' results back
    D1 = E.detrend_observed(3, niter=2)
    resid = runs(E, P)
    R1 = E.highpass_observed()
    assert same_bits(R1.data, xcor.highpass_observed_reference(D1.data, ob.weight, ob.seg_first, HP)[0]) and not same_bits(R1.data, R0.data)
    hp_runs = runs(E, P)
    assert not same_runs(hp_runs, resid)
    assert same_bits(E.highpass_observed().data, R1.data) and same_runs(runs(E, P), hp_runs)
    E.highpass_observed(apply=False)
    assert same_runs(runs(E, P), resid)
    # detrend, high-pass, detrend: the second detrend is a fresh handle's single one, and so is what follows it
    E.highpass_observed()
    D2 = E.detrend_observed(3, niter=2)
    F = case.handle(ob, hp=HP)
    DF = F.detrend_observed(3, niter=2)
    assert oc.same_detrend(D2, DF) and oc.same_detrend(D2, D1)
    assert same_runs(runs(E, P), runs(F, P)) and same_runs(runs(E, P), resid)
    F.close()
    # a high-pass over the residuals, then the detrend's undo: the raw set, and the high-pass gone with it
    E.highpass_observed()
    E.detrend_observed(0)
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), raw_runs)
    E.highpass_observed(apply=False)
    assert same_bits(E.run_moments(P.atm, P.opts, SHIFTS), raw_runs)
    # set_highpass of another table, or of none, afterwards changes no datum: the undo needs no high-pass either
    E.detrend_observed(3, niter=2, outputs=False)
    E.highpass_observed(outputs=False)
    E.set_highpass(None)
    other = runs(E, P)
    G = case.handle(xcor.Observed(ob.seg_first, R1.data, ob.weight, ob.gain))
    G.set_weighted_filter(xcor.WeightedFilter(D1.basis))
    assert same_runs(other, runs(G, P))
    box = hc.tables(5)["boxcar"]
    E.set_highpass(box)
    G.set_highpass(box)
    assert same_runs(runs(E, P), runs(G, P))
    G.close()
    E.set_highpass(None)
    E.highpass_observed(apply=False)
    assert not same_runs(runs(E, P), other)                  # (the undo needs no high-pass: the residuals are back)
    E.set_highpass(HP)
    assert same_runs(runs(E, P), resid)
    # set_observed drops everything
    E.highpass_observed()
    ob12 = case.observed(12, weighted)
    E.set_observed(ob12)
    E.set_highpass(HP)
    assert same_bits(E.highpass_observed().data, xcor.highpass_observed_reference(ob12.data, ob12.weight, ob12.seg_first, HP)[0])
    E.close()


def test_the_weigh_reads_the_high_passed_data_and_keeps_its_weights(case):
    P = case.P
    ob = case.observed(7, True)
    E = case.handle(ob, hp=HP)
    D = E.detrend_observed(3, niter=2)
    R = E.highpass_observed()
    # detrend, high-pass, weigh: the scatter of r' under W
    Wg = E.weigh_observed(V, clip=3.0)
    var, med, keep, w1 = xcor.scatter_reference(R.data, ob.weight, ob.seg_first, V, 3.0, 2)
    assert same_bits(Wg.variance, var) and same_bits(Wg.median, med) and same_bits(Wg.weight, w1)
    weighed = runs(E, P)
    F = case.handle(xcor.Observed(ob.seg_first, R.data, w1, ob.gain))
    assert F.set_weighted_filter(xcor.WeightedFilter(D.basis)) == Wg.nsingular
    F.set_highpass(HP)
    assert same_runs(weighed, runs(F, P))
    F.close()
    # a high-pass call after the weigh: the weights in force stay, and it reads W, not w' -- the same r'
    again = E.highpass_observed()
    assert same_bits(again.data, R.data) and again.ndead == R.ndead and same_runs(runs(E, P), weighed)
    # the weigh's undo does not touch the data
    E.weigh_observed(xcor.SCATTER_NONE)
    G = case.handle(xcor.Observed(ob.seg_first, R.data, ob.weight, ob.gain), hp=HP)
    G.set_weighted_filter(xcor.WeightedFilter(D.basis))
    assert same_runs(runs(E, P), runs(G, P))
    G.close()
    E.close()
    # weigh, then high-pass, under a plain filter over the raw set: weights and filter stay as they were
    filt = xcor.svd_filter(ob.data, ob.seg_first, 2)
    E = case.handle(ob, hp=HP)
    E.set_filter(filt)
    W0 = E.weigh_observed(V, clip=3.0)
    R0 = E.highpass_observed()
    assert same_bits(R0.data, xcor.highpass_observed_reference(ob.data, ob.weight, ob.seg_first, HP)[0])
    H = case.handle(xcor.Observed(ob.seg_first, R0.data, W0.weight, ob.gain), hp=HP)
    H.set_filter(filt)
    assert same_runs(runs(E, P), runs(H, P))
    H.close()
    E.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(case):
    P = case.P
    ob = case.observed(7, True)
    E = case.handle(ob, hp=HP)
    E.detrend_observed(3, niter=2)
    good = E.highpass_observed()
    ref = runs(E, P)
    lib, dp = E._lib, _abi.c_double_p
    data, nd = np.full((7, 800), -7.0), C.c_int64(-7)

    def raw(X, apply):
        rc = lib.trx_highpass_observed(X._h, apply, data.ctypes.data_as(dp), C.byref(nd))
        assert np.all(data == -7.0) and nd.value == -7      # a refusal touches no output
        return rc, X._last_error()

    who = "trx_highpass_observed: "
    for apply in (2, -1, 7):
        assert raw(E, apply) == (-1, who + "apply must be 0 (undo) or 1")
    assert same_runs(runs(E, P), ref)
    # no high-pass installed: apply = 1 is refused, apply != 0, 1 is named first, and the undo goes through
    E.set_highpass(None)
    assert raw(E, 1) == (-1, who + "no high-pass installed (trx_set_highpass)")
    assert raw(E, 2) == (-1, who + "apply must be 0 (undo) or 1")
    E.set_highpass(HP)
    assert same_runs(runs(E, P), ref)
    again = E.highpass_observed()
    assert same_bits(again.data, good.data)
    E.close()
    # no observed set: named ahead of everything else
    N = case.handle(None)
    for apply in (1, 0, 2):
        assert raw(N, apply) == (-1, who + "no observed set installed (trx_set_observed)")
    with pytest.raises(EngineError) as ei:
        N.highpass_observed()
    assert ei.value.code == -1 and who + "no observed set installed (trx_set_observed)" in str(ei.value)
    N.close()
    # a shard of the grid
    n = P.nwn
    try:
        P.set_shard(1000, 3000)
        S = Engine(P.static)
        S.set_pixels(pixels.Pixels([2510.0, 2520.0, 2530.0, 2540.0], [0.2, 0.3, 1.5, 0.4], 4.0))
        S.set_observed(xcor.Observed([0, 1, 4], np.ones((7, 4))))
        S.set_highpass(xcor.boxcar_highpass(3))
        for apply in (True, False):
            with pytest.raises(EngineError) as ei:
                S.highpass_observed(apply=apply)
            assert ei.value.code == -6 and who + "this handle's shard is not the whole grid" in str(ei.value)
        assert raw(S, 2) == (-1, who + "apply must be 0 (undo) or 1")
        S.close()
    finally:
        P.set_shard(0, n)


# ---- 6. injection, detrend, high-pass, weigh and recovery, end to end -----------------------------------------------
def test_injection_high_pass_weights_and_recovery_end_to_end(case):
    """test_gpu_scatter's end-to-end set -- a continuum with smooth trends in time plus seeded noise, two segments, five
    columns of 10 x the noise -- on a handle with a high-pass installed: the model is injected at the cell (Kp, Vsys) =
    (100, 6) km/s of test_gpu_trail's 5 x 5 map, SYSREM takes two components, the residuals go through the model's own
    high-pass, the columns are weighed by their inverse variance with a clip of 3, and the CCF map of trx_run_exposed_map,
    whose model goes through the same high-pass, is the recovery."""
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
    hp = xcor.gaussian_highpass(25.0)
    vm = xc.the_map("ccf", kp=xc.TRAIL_KP, vsys=xc.TRAIL_VSYS)
    cell = (int(np.argmin(np.abs(xc.TRAIL_KP - xc.KP_TRUE))), int(np.argmin(np.abs(xc.TRAIL_VSYS - xc.VSYS_TRUE))))
    assert cell == (2, 3) and (vm.nkp, vm.nvsys) == (5, 5)
    shifts = np.array([pixels.shift(v) for v in xc.VSYS_TRUE + xc.KP_TRUE * xc.ORBIT])
    p0 = 0.1 / case.scale
    E = case.handle(ob, hp=hp)
    E.set_exposures(Exposures(np.ones(7), np.full(7, 2e-6)))

    def peak(m):
        assert np.isfinite(m).all()
        return tuple(int(i) for i in np.unravel_index(np.argmax(m), m.shape))

    def margin(m):
        """how far the first cell stands above the second, in units of the other cells' scatter"""
        order = np.sort(m.reshape(-1))
        return float((order[-1] - order[-2]) / np.std(order[:-1]))

    # the precondition, on the host from the device's pairs: the numpy chain alone -- inject, SYSREM, high-pass, weigh, map --
    # finds the injected cell, and does not without the injection
    injected = E.run_exposed(P.atm, P.opts, shifts)
    pairs_lv = np.stack([E.run_exposed(P.atm, P.opts, np.full(7, s)) for s in xc.LAGS])

    def host_map(data):
        basis, coef, resid = xcor.sysrem_reference(data, w, seg, 2, 10)
        hpd, ndead = xcor.highpass_observed_reference(resid, w, seg, hp)
        var, med, keep, w1 = xcor.scatter_reference(hpd, w, seg, V, 3.0, 2)
        return xcor.exposed_map_reference(pairs_lv, xcor.Observed(seg, hpd, w1, ob.gain), xcor.WeightedFilter(basis), vm, hp), (hpd, ndead, var, med, w1)

    (with_injection, mirror), (without, _) = host_map(xcor.inject_reference(injected, ob, p0, 1.0)), host_map(raw)
    print("numpy chain, injected (rows Kp, columns Vsys):\n%s\nnumpy chain, not injected:\n%s"
          % (np.array2string(with_injection, precision=4), np.array2string(without, precision=4)))
    print("numpy chain: the injected cell leads by %.2f of the other cells' scatter" % margin(with_injection))
    assert peak(with_injection) == cell and peak(without) != cell
    # the device
    E.detrend_observed(2, 10, inject=(P.atm, P.opts, shifts, p0, 1.0), outputs=False)
    H = E.highpass_observed()
    assert same_bits(H.data, mirror[0]) and H.ndead == mirror[1] == np.count_nonzero(w == 0)
    R = E.weigh_observed(V, clip=3.0)
    assert same_bits(R.variance, mirror[2]) and same_bits(R.median, mirror[3]) and same_bits(R.weight, mirror[4])
    print("%d entries dead, %d columns clipped (%s of the five noisy ones among them), %d dead in the filter"
          % (H.ndead, R.nmasked, sum(R.weight[:, p].max() == 0 for p in noisy), R.nsingular))
    assert 5 <= R.nmasked < 400
    m, idx = E.run_exposed_map(P.atm, P.opts, vm, lag_index=True)
    print("device (rows Kp, columns Vsys):\n%s\ndevice: the injected cell leads by %.2f of the other cells' scatter" % (np.array2string(m, precision=4), margin(m)))
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
def full_wave_share(w, seg, half):
    """the share of the kernel's waves that take the full-window path: a wave owns the outputs [o, o + 64) and [o + 256, o + 320)
    of a tile of 512, and is full if every entry of their windows is live and inside the segment"""
    nexp, npix = w.shape
    dead = np.concatenate([np.zeros((nexp, 1)), np.cumsum(w <= 0, axis=1)], axis=1)      # dead[:, q]: dead entries below q
    waves = full = 0
    for s in range(len(seg) - 1):
        a, b = int(seg[s]), int(seg[s + 1])
        for first in range(a, b, hc.TILE):
            count = min(hc.TILE, b - first)
            for w0 in range(0, min(256, count), 64):
                ok = np.ones(nexp, dtype=bool)
                for o in (w0, w0 + 256):
                    if o < count:
                        lo, hi = first + o - half, first + min(o + 64, count) + half
                        ok &= (dead[:, min(hi, npix)] - dead[:, max(lo, 0)] == 0) if lo >= a and hi <= b else False
                waves += nexp
                full += int(np.count_nonzero(ok))
    return full / waves


def test_size_and_time(case):
    """40 orders of 2048 pixels, 100 exposures, 2 % masked, a Gaussian table of sigma 80 cut at 3 sigma (half 240), a warm
    handle: the device call with its output left on the device (a host clock around calls that return synchronised, after
    one warm-up call, the mean of 20) must be faster than xcor.highpass_observed_reference on the host, measured here; a
    window walk that loses to numpy means a mis-sized launch.  detrend_observed(5, 10) alone is printed for scale, and the
    kernel's fp64 floor: 4 (2 half + 1) operations per entry on the masked path, half that on the full path, at 256 CUs x 64
    lanes per clock x 2.4 GHz."""
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
    hp = xcor.gaussian_highpass(80.0)
    assert hp.half == 240
    E = Engine(P.static)
    E.set_pixels(px)
    E.set_observed(xcor.Observed(seg, raw, w))
    E.set_highpass(hp)
    D = E.detrend_observed(5, 10)                            # (the warm-up of the detrend, and the residuals to high-pass)
    t0 = time.perf_counter()
    for _ in range(reps):
        E.detrend_observed(5, 10, outputs=False)
    t_detrend = (time.perf_counter() - t0) / reps
    first = E.highpass_observed()                            # (the warm-up)
    t0 = time.perf_counter()
    for _ in range(reps):
        E.highpass_observed(outputs=False)
    t_device = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    want, ndead = xcor.highpass_observed_reference(D.data, w, seg, hp)
    t_host = time.perf_counter() - t0
    assert same_bits(first.data, want) and first.ndead == ndead == np.count_nonzero(w == 0)
    assert same_bits(E.highpass_observed().data, first.data)
    E.close()
    share = full_wave_share(w, seg, hp.half)
    per_entry = 4.0 * (2 * hp.half + 1) * (1.0 - 0.5 * share)
    floor = per_entry * nexp * npix / (256 * 64 * 2.4e9)
    print("40 x 2048 pixels, 100 exposures, half 240:")
    print("  %-64s %9.3f ms" % ("highpass_observed on the device, output left there", 1e3 * t_device))
    print("  %-64s %9.3f ms" % ("xcor.highpass_observed_reference on the host", 1e3 * t_host))
    print("  %-64s %9.3f ms" % ("detrend_observed(5, 10) alone, for scale", 1e3 * t_detrend))
    print("  %-64s %9.3f ms (the call: %.2f times)" % ("the kernel's fp64 floor", 1e3 * floor, t_device / floor))
    print("  ndead %d; %.2f %% of the waves on the full-window path" % (first.ndead, 100.0 * share))
    assert t_device < t_host
