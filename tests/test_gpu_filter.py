"""The detrending filter between the detector pixels and their moments on the device (trx_set_filter /
trx_run_filtered_moments and the batch forms, include/transit_hip.h) against transit_amd.xcor, the numpy statement of
the same definition.

The case is pixel_cases.make's (6001 bins, 60 layers; 20 000 lines where only bits are compared), the seven shifts its
own, the pixel set the 800-pixel set of xcor_checks with its two off-grid pixels -- and one further pixel of set A
moved to 2561.0 cm-1: at these shifts its window is on the grid at -150 km/s only, so its pairs have b > 0 at one
exposure and its column is dead all the same.  Segment lengths [1, 63, 64, 65, 200, 0, 7, 400]: tiles of 1, 63, 64 and
64 + 1 pixels, an empty segment, and 400 = 6 tiles + 16.

Tolerances, both derived, not measured.
Values, per element, relative to xcor.filter_abs_reference A = |g| + |back| (|fwd| |g|): (nexp + ncomp + 8) * 2^-52 --
two roundings in g, nexp products and sums in a coefficient, ncomp in the projection, one subtraction, doubled to leave
room for the reference's own rounding.
Moments: compared with xcor.reference_values over the VALUES THE DEVICE RETURNED (so that the cancellation inside g'
does not enter), by the rule of xcor_checks.check_moments: (n_max + 16) * 2^-52 of the sums of absolute terms, the count exact."""
import ctypes as C
import math
import os
import shutil

import numpy as np
import pytest

import pixel_cases as pc
import xcor_checks as xc
from cases import GOLDEN
from transit_amd import _abi, pixels, xcor
from transit_amd.engine import Batch, Engine, EngineError
from transit_amd.host import Problem

pytestmark = pytest.mark.gpu

SHIFTS = pc.SHIFTS


@pytest.mark.parametrize("solution", ["eclipse", "transit"])
def test_filtered_values_and_moments_are_the_definition(tmp_path, solution):
    P = pc.make(tmp_path, solution)
    assert P.nwn == 6001
    px = xc.straddle_pixel_set(P)
    plain, E = Engine(P.static), Engine(P.static)
    ob = xc.observed(len(px), float(np.mean(plain.run(P.atm, P.opts)["spectrum"])))
    F = xcor.svd_filter(ob.data, ob.seg_first, 3)
    assert (F.nseg, F.ncomp, F.nexp) == (8, 3, 7)
    E.set_pixels(px)
    E.set_observed(ob)
    E.set_filter(F)
    deep, keep = pc.thinner(P, 1e-3)
    for k, atm in enumerate((P.atm, P.atm, deep, P.atm)):      # fresh, hinted, resuming deeper, hinted again
        what = "%s run %d" % (solution, k)
        spec_ref = plain.run(atm, P.opts)["spectrum"]
        pairs = E.run_pixels(atm, P.opts, SHIFTS)
        mom, spec, val = E.run_filtered_moments(atm, P.opts, SHIFTS, spectrum=True, values=True)
        assert np.array_equal(spec, spec_ref), what
        for p in xc.STRADDLE:                             # on the grid at exactly one shift
            assert np.count_nonzero(pairs[:, p, 1] > 0) == 1 and pairs[0, p, 1] > 0
        for p in xc.OFF_GRID:
            assert np.all(pairs[:, p, 1] == 0)
        xc.check_values(val, pairs, ob, F, what)
        assert np.flatnonzero(np.isnan(val).any(axis=0)).tolist() == xc.DEAD and np.isnan(val[:, xc.DEAD]).all(), what
        xc.check_filtered_moments(mom, val, ob, what)
        # without the values, without the spectrum: the same moments
        assert np.array_equal(E.run_filtered_moments(atm, P.opts, SHIFTS), mom), what
    plain.close(); E.close()


def test_an_all_zero_filter_gives_the_unfiltered_bits(tmp_path):
    P = pc.make(tmp_path, "eclipse", nlines=20_000)
    px = xc.straddle_pixel_set(P, straddle=False)
    E = Engine(P.static)
    E.set_pixels(px)
    ob = xc.observed(len(px), float(np.mean(E.run(P.atm, P.opts)["spectrum"])))
    E.set_observed(ob)
    E.set_filter(xcor.Filter(np.zeros((ob.nseg, 1, ob.nexp)), np.zeros((ob.nseg, ob.nexp, 1))))
    pairs = E.run_pixels(P.atm, P.opts, SHIFTS)
    mom, val = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    off = sorted(xc.OFF_GRID)
    on = np.ones(len(px), dtype=bool)
    on[off] = False
    assert np.all(pairs[:, on, 1] > 0) and np.all(pairs[:, off, 1] == 0)
    g = ob.gain[None, on] * (pairs[:, on, 0] / pairs[:, on, 1])
    assert np.array_equal(val[:, on], g) and np.isnan(val[:, off]).all()
    assert np.array_equal(mom, E.run_moments(P.atm, P.opts, SHIFTS))
    E.close()


@pytest.mark.parametrize("ncomp", [1, 5, 16])
def test_random_filters_of_every_register_size(tmp_path, ncomp):
    """ncomp 1, 5 and 16 take the kernel's instantiations for 4, 8 and 16 components"""
    P = pc.make(tmp_path, "transit", nlines=20_000)
    px = xc.straddle_pixel_set(P)
    E = Engine(P.static)
    E.set_pixels(px)
    ob = xc.observed(len(px), float(np.mean(E.run(P.atm, P.opts)["spectrum"])), seed=5)
    E.set_observed(ob)
    F = xc.random_filter(ob.nseg, ncomp, ob.nexp, seed=ncomp)
    assert F.fwd.min() < 0 < F.fwd.max() and F.back.min() < 0 < F.back.max()
    E.set_filter(F)
    pairs = E.run_pixels(P.atm, P.opts, SHIFTS)
    mom, val = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    xc.check_values(val, pairs, ob, F, "ncomp %d" % ncomp)
    assert np.flatnonzero(np.isnan(val).any(axis=0)).tolist() == xc.DEAD
    xc.check_filtered_moments(mom, val, ob, "ncomp %d" % ncomp)
    # the same filter padded with zero components to the next instantiation: the same bits
    if ncomp < 16:
        wide = {1: 5, 5: 9}[ncomp]
        fwd, back = np.zeros((ob.nseg, wide, ob.nexp)), np.zeros((ob.nseg, ob.nexp, wide))
        fwd[:, :ncomp], back[:, :, :ncomp] = F.fwd, F.back
        E.set_filter(xcor.Filter(fwd, back))
        mom2, val2 = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
        assert np.array_equal(val2, val, equal_nan=True) and np.array_equal(mom2, mom)
    E.close()


def test_bits_do_not_depend_on_the_rest_of_the_call(tmp_path):
    P = pc.make(tmp_path, "eclipse", nlines=20_000)
    px = xc.straddle_pixel_set(P)
    E = Engine(P.static)
    E.set_pixels(px)
    ob = xc.observed(len(px), float(np.mean(E.run(P.atm, P.opts)["spectrum"])))
    E.set_observed(ob)
    F = xc.random_filter(ob.nseg, 3, ob.nexp, seed=1)
    E.set_filter(F)
    mom, val = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    assert np.all(mom[:, 5] == 0) and np.all(mom[:, [0, 1, 2, 3, 4, 6, 7], 0] > 0)
    for _ in range(2):
        m, v = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
        assert np.array_equal(m, mom) and np.array_equal(v, val, equal_nan=True)
    # the same pixels cut into other segments, more of them: a segment that keeps its pixels AND its matrices keeps its
    # values and its rows, while every other segment's matrices change
    lengths = [1, 30, 33, 64, 65, 100, 100, 0, 0, 7, 150, 250]
    again = xcor.Observed(xcor.segments(lengths), ob.data, ob.weight, ob.gain)
    same = {0: 0, 3: 2, 4: 3, 7: 5, 8: 5, 9: 6}              # new segment -> the old one of the same pixels
    G = xc.random_filter(again.nseg, 3, again.nexp, seed=2)
    for new, old in same.items():
        assert again.seg_first[new:new + 2].tolist() == ob.seg_first[old:old + 2].tolist()
        G.fwd[new], G.back[new] = F.fwd[old], F.back[old]
    E.set_observed(again)
    E.set_filter(G)
    mom2, val2 = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    assert mom2.shape == (7, 12, 7)
    for new, old in same.items():
        a, z = again.seg_first[new:new + 2]
        assert np.array_equal(val2[:, a:z], val[:, a:z], equal_nan=True), (new, old)
        assert np.array_equal(mom2[:, new], mom[:, old]), (new, old)
    for new in (1, 2, 5, 6, 10, 11):
        a, z = again.seg_first[new:new + 2]
        live = ~np.isnan(val[0, a:z])
        assert np.all(val2[:, a:z][:, live] != val[:, a:z][:, live]), new
    # through a batch of two ways: each atmosphere's bits are the single handle's
    K = 3
    atms, keep = pc.atmospheres(P, K)
    shifts = np.stack([np.roll(SHIFTS, j) * (1.0 + 1e-6 * j) for j in range(K)])
    E.set_observed(ob)
    E.set_filter(F)
    ref = np.stack([E.run_filtered_moments(atms[j], P.opts, shifts[j]) for j in range(K)])
    assert len({ref[j].tobytes() for j in range(K)}) == K
    E.close()
    B = Batch(P.static, ways=2)
    B.set_pixels(px)
    B.set_observed(ob)
    B.set_filter(F)
    for rep in range(2):
        got = B.run_filtered_moments(atms, P.opts, shifts)
        assert got.shape == (K, 7, 8, 7) and np.array_equal(got, ref), rep
    B.close()


def test_the_other_runs_do_not_know_of_the_filter(tmp_path):
    P = pc.make(tmp_path, "eclipse", nlines=20_000)
    px = xc.straddle_pixel_set(P)
    E, bare = Engine(P.static), Engine(P.static)
    ob = xc.observed(len(px), float(np.mean(bare.run(P.atm, P.opts)["spectrum"])))
    for X in (E, bare):
        X.set_pixels(px)
        X.set_observed(ob)
    E.set_filter(xc.random_filter(ob.nseg, 8, ob.nexp, seed=4))
    for k in range(2):
        E.run_filtered_moments(P.atm, P.opts, SHIFTS)
        assert np.array_equal(E.run_pixels(P.atm, P.opts, SHIFTS), bare.run_pixels(P.atm, P.opts, SHIFTS)), k
        assert np.array_equal(E.run_moments(P.atm, P.opts, SHIFTS), bare.run_moments(P.atm, P.opts, SHIFTS)), k
        assert np.array_equal(E.run(P.atm, P.opts)["spectrum"], bare.run(P.atm, P.opts)["spectrum"]), k
    E.close(); bare.close()


def test_likelihood_end_to_end(tmp_path):
    """xcor.loglike_bl19_sum of the filtered moments against the direct evaluation (means subtracted first) on the
    values the device returned, row by row to the 1e-10 of test_gpu_moments, the sum to 1e-10 of the sum of the rows'
    absolute values"""
    P = pc.make(tmp_path, "transit", nlines=20_000)
    px = xc.straddle_pixel_set(P)
    E = Engine(P.static)
    E.set_pixels(px)
    ob = xc.observed(len(px), float(np.mean(E.run(P.atm, P.opts)["spectrum"])), seed=9)
    E.set_observed(ob)
    E.set_filter(xcor.svd_filter(ob.data, ob.seg_first, 3))
    mom, val = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    use = ~np.isnan(val) & (ob.weight > 0)
    f, w, g = ob.data, ob.weight, val
    ll = xcor.loglike_bl19(mom)
    worst, total, size = 0.0, [], []
    for v in range(ob.nexp):
        for s in range(ob.nseg):
            k = np.arange(ob.seg_first[s], ob.seg_first[s + 1])
            k = k[use[v, k]]
            if k.size < 2:
                assert math.isnan(ll[v, s])
                continue
            sw = math.fsum(w[v, k])
            mf, mg = math.fsum(w[v, k] * f[v, k]) / sw, math.fsum(w[v, k] * g[v, k]) / sw
            sf2 = math.fsum(w[v, k] * (f[v, k] - mf) ** 2) / sw
            sg2 = math.fsum(w[v, k] * (g[v, k] - mg) ** 2) / sw
            r = math.fsum(w[v, k] * (f[v, k] - mf) * (g[v, k] - mg)) / sw
            want = -0.5 * k.size * math.log(sf2 - 2 * r + sg2)
            assert math.isfinite(ll[v, s])
            worst = max(worst, abs(ll[v, s] - want) / abs(want))
            total.append(want); size.append(abs(want))
    got, want = xcor.loglike_bl19_sum(mom), math.fsum(total)
    print("loglike_bl19: worst relative difference of a row %.3e, of the sum over the rows' absolute values %.3e (tolerance 1e-10)"
          % (worst, abs(got - want) / math.fsum(size)))
    assert worst <= 1e-10
    assert abs(got - want) <= 1e-10 * math.fsum(size)
    assert np.isnan(ll).sum() >= 2 * ob.nexp
    E.close()


def test_opacity_grid_handle(tmp_path):
    d = tmp_path / "og"
    shutil.copytree(os.path.join(GOLDEN, "opacity_grid"), d)
    P = Problem.from_cfg(os.path.join(str(d), "case.cfg"))
    builder = Engine(P.static)
    builder.build_opacity_grid(P)
    builder.close()
    assert P.static.ogrid
    wn_i, wn_d, n, wn = pc.grid(P)
    centres = np.linspace(wn[0] + 1.0, wn[-1] - 1.0, 25) + 0.37 * wn_d
    px = pc.joined(pixels.resolving_power(centres, 1000.0), pixels.resolving_power(centres, 100.0))
    shifts = np.array([1.0, 1.0 - 150.0 / 299792.458, 1.0 + 150.0 / 299792.458, 0.9991])
    plain, E = Engine(P.static), Engine(P.static)
    E.set_pixels(px)
    ob = xc.observed(len(px), float(np.mean(plain.run(P.atm, P.opts)["spectrum"])), lengths=[10, 0, 15, 25], nexp=4)
    E.set_observed(ob)
    F = xcor.svd_filter(ob.data, ob.seg_first, 2)
    E.set_filter(F)
    for k in range(2):
        ref = plain.run(P.atm, P.opts)["spectrum"]
        pairs = E.run_pixels(P.atm, P.opts, shifts)
        mom, spec, val = E.run_filtered_moments(P.atm, P.opts, shifts, spectrum=True, values=True)
        assert np.array_equal(spec, ref)
        xc.check_values(val, pairs, ob, F, "opacity grid run %d" % k)
        xc.check_filtered_moments(mom, val, ob, "opacity grid run %d" % k)
        assert np.array_equal(E.run(P.atm, P.opts)["spectrum"], ref)
    plain.close(); E.close()


def test_refusals_and_lifetimes(tmp_path):
    P = pc.make(tmp_path, "eclipse", nlines=10_000)
    sh = np.ascontiguousarray(SHIFTS[:3])
    good_px = pixels.Pixels([2510.0, 2520.0, 2530.0, 2540.0], [0.2, 0.3, 1.5, 0.4], 4.0)
    rng = np.random.default_rng(2)
    f, w, gain = rng.standard_normal((3, 4)), rng.uniform(0.5, 2.0, (3, 4)), rng.uniform(0.5, 1.5, 4)
    good_ob = xcor.Observed([0, 1, 4], f, w, gain)
    good = xc.random_filter(2, 2, 3, seed=6)
    E = Engine(P.static)
    lib = E._lib
    dp = _abi.c_double_p

    def refusal(X, filt):
        with pytest.raises(EngineError) as ei:
            X.set_filter(filt)
        assert ei.value.code == -1
        return str(ei.value)

    assert "observed" in refusal(E, good)                              # no pixel set, no observed set
    E.set_pixels(good_px)
    assert "observed" in refusal(E, good)                              # no observed set to install it over
    E.set_observed(good_ob)
    with pytest.raises(EngineError) as ei:                             # no filter
        E.run_filtered_moments(P.atm, P.opts, sh)
    assert ei.value.code == -1 and "filter" in str(ei.value)
    E.set_filter(good)
    before, vbefore = E.run_filtered_moments(P.atm, P.opts, sh, values=True)
    assert before.shape == (3, 2, 7) and np.array_equal(before[..., 0], [[1, 3]] * 3) and not np.isnan(vbefore).any()
    assert not np.array_equal(before, E.run_moments(P.atm, P.opts, sh))

    def unchanged(what):
        assert np.array_equal(E.run_filtered_moments(P.atm, P.opts, sh), before), what

    def changed(which, idx, val):
        arrs = {"fwd": good.fwd.copy(), "back": good.back.copy()}
        arrs[which][idx] = val
        return xcor.Filter(**arrs)

    for what, filt, name in (("fwd nan", changed("fwd", (1, 0, 2), np.nan), "segment 1"),
                             ("fwd inf", changed("fwd", (0, 1, 0), np.inf), "segment 0"),
                             ("back nan", changed("back", (0, 2, 1), np.nan), "segment 0"),
                             ("back -inf", changed("back", (1, 0, 0), -np.inf), "segment 1"),
                             ("17 components", xc.random_filter(2, 17, 3, seed=7), "TRX_FILTER_MAX")):
        assert name in refusal(E, filt), what
        unchanged(what)
    assert "fwd" in refusal(E, changed("fwd", (1, 0, 2), np.nan)) and "back" in refusal(E, changed("back", (1, 0, 0), np.nan))

    def raw(**kw):
        c = good.to_c()
        for k, v in kw.items():
            setattr(c, k, v)
        return lib.trx_set_filter(E._h, C.byref(c)), lib.trx_last_error(E._h)

    assert raw(ncomp=-1) == (-1, b"filter: ncomp < 0")
    assert raw(ncomp=17)[0] == -1 and b"TRX_FILTER_MAX" in raw(ncomp=17)[1]
    assert raw(fwd=None)[0] == -1 and raw(back=None)[0] == -1 and b"NULL" in raw(back=None)[1]
    unchanged("raw refusals")
    # the run's own refusals
    out = np.zeros_like(before)

    def run(nshift, shift, dest):
        return lib.trx_run_filtered_moments(E._h, C.byref(P.atm), C.byref(P.opts), None, nshift,
                                            shift.ctypes.data_as(dp) if shift is not None else None, None,
                                            dest.ctypes.data_as(dp) if dest is not None else None, None)

    assert run(2, sh, out) == -1 and b"nexp" in lib.trx_last_error(E._h)
    assert run(4, np.ascontiguousarray(SHIFTS[:4]), np.zeros((4, 2, 7))) == -1 and run(0, sh, out) == -1
    assert run(3, None, out) == -1 and run(3, sh, None) == -1 and b"mom is NULL" in lib.trx_last_error(E._h)
    for what, v in (("nan", np.nan), ("inf", np.inf), ("0", 0.0), ("< 0", -1.0)):
        s = sh.copy()
        s[1] = v
        assert run(3, s, out) == -1, what
        assert b"shift 1 must be finite and > 0" in lib.trx_last_error(E._h), what
    assert np.all(out == 0)
    assert run(3, sh, out) == 0 and np.array_equal(out, before)
    # a refused set_observed or set_pixels keeps the filter; a successful set_observed drops it, a clearing one too
    with pytest.raises(EngineError):
        E.set_observed(xcor.Observed([0, 3, 2, 4], f, w, gain))
    with pytest.raises(EngineError):
        E.set_pixels(pixels.Pixels([2510.0, 2520.0, 2530.0, 2540.0], [0.2, 0.3, 0.0, 0.4], 4.0))
    unchanged("refused sets")
    E.set_observed(good_ob)
    with pytest.raises(EngineError) as ei:
        E.run_filtered_moments(P.atm, P.opts, sh)
    assert ei.value.code == -1 and "filter" in str(ei.value)
    E.set_filter(good)
    unchanged("installed again")
    E.set_observed(None)
    assert run(3, sh, out) == -1 and "observed" in refusal(E, good)
    E.set_observed(good_ob)
    E.set_filter(good)
    E.set_pixels(good_px)                              # drops both
    assert run(3, sh, out) == -1 and b"observed" in lib.trx_last_error(E._h)
    assert "observed" in refusal(E, good)
    E.set_observed(good_ob)
    assert run(3, sh, out) == -1 and b"filter" in lib.trx_last_error(E._h)
    E.set_filter(good)
    unchanged("after set_pixels")
    E.set_filter(None)                                 # cleared: refused again; ncomp = 0 clears too
    assert run(3, sh, out) == -1
    E.set_filter(good)
    assert raw(ncomp=0)[0] == 0 and run(3, sh, out) == -1 and b"filter" in lib.trx_last_error(E._h)
    E.close()
    # a shard's partial pairs say nothing about the filtered moments
    n = P.nwn
    try:
        P.set_shard(1000, 3000)
        S = Engine(P.static)
        S.set_pixels(good_px)
        S.set_observed(good_ob)
        S.set_filter(good)
        with pytest.raises(EngineError) as ei:
            S.run_filtered_moments(P.atm, P.opts, sh)
        assert ei.value.code == -6 and "trx_run_pixels" in str(ei.value)
        assert S.run_pixels(P.atm, P.opts, sh).shape == (3, 4, 2)
        S.close()
    finally:
        P.set_shard(0, n)
    # a batch installs a filter on every handle or on none
    B = Batch(P.static, ways=2)
    three = np.stack([sh] * 3)
    assert "observed" in refusal(B, good)
    B.set_pixels(good_px)
    B.set_observed(good_ob)
    with pytest.raises(EngineError) as ei:
        B.run_filtered_moments([P.atm], P.opts, three[:1])
    assert "filter" in str(ei.value)
    B.set_filter(good)
    ref = B.run_filtered_moments([P.atm, P.atm, P.atm], P.opts, three)
    assert np.array_equal(ref[0], before) and np.array_equal(ref[2], before)
    assert "segment 1" in refusal(B, changed("fwd", (1, 0, 2), np.nan))
    assert np.array_equal(B.run_filtered_moments([P.atm, P.atm, P.atm], P.opts, three), ref)
    with pytest.raises(EngineError) as ei:             # a bad shift of one atmosphere fails the call and names it
        worse = three.copy()
        worse[1, 2] = 0.0
        B.run_filtered_moments([P.atm, P.atm, P.atm], P.opts, worse)
    assert "shift 2" in str(ei.value)
    with pytest.raises(EngineError):                   # nshift != nexp
        B.run_filtered_moments([P.atm], P.opts, np.stack([SHIFTS[:2]]))
    B.set_observed(good_ob)                            # drops it on every handle
    with pytest.raises(EngineError):
        B.run_filtered_moments([P.atm], P.opts, three[:1])
    B.close()
