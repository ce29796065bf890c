"""Cross-correlation moments of the detector pixels against observed data on the device (trx_set_observed /
trx_run_moments and the batch forms, include/transit_hip.h) against transit_amd.xcor, the numpy statement of the
same definition.

The case is pixel_cases.make's (40 000 lines, 6001 bins, 60 layers), the pixel set its 800-pixel joined set A + B
(windows of 42-44 and of 283-290 bins: both forms of the pair kernel), the shifts its seven.  Two of the 800 pixels
(one in A, one in B) are moved off the grid, to 2400 and 2700 cm-1: their pairs have b = 0 and count in no moment.
Segment lengths [1, 63, 64, 65, 200, 0, 7, 400]: one lane, a wave less one, a wave, a wave plus one, several
strides, an empty segment, a short one, the longest; 7 exposures x 8 segments = 56 waves, the last block ragged.
(A second segmentation, [300, 200, 300], has a segment with windows of both forms in it.)  The exposure and the order axis
-- 64, 65 and 130 exposures, 64, 65 and 130 segments -- are test_gpu_many_exposures.py's.

Tolerance of the accuracy checks, per moment, relative to xcor.abs_reference (the same sum over |terms|):
(n_max + 16) * 2^-52 with n_max the longest segment -- the worst case of a double sum of n terms, (n - 1) * 2^-53
each way it is ordered, with each term made of at most four correctly rounded operations (a / b, gain *, w *, * g),
4 * 2^-53 more, rounded up generously; derived, not measured.  chi2 from moments adds the rounding of six products and
five additions on sums of that accuracy and is compared with a direct numpy evaluation that has a few roundings per
term of its own: (n_max + 32) * 2^-52 of the sum of w (|f| + |a| |g| + |b|)^2."""
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
def test_moments_are_the_definition_over_the_pixel_pairs(tmp_path, solution):
    P = pc.make(tmp_path, solution)
    assert P.nwn == 6001
    px = xc.pixel_set(P)
    plain, E, only = Engine(P.static), Engine(P.static), Engine(P.static)
    scale = float(np.mean(plain.run(P.atm, P.opts)["spectrum"]))
    ob = xc.observed(len(px), scale)
    assert (ob.nexp, ob.nseg) == (7, 8) and np.count_nonzero(ob.weight == 0) > 100
    for X in (E, only):
        X.set_pixels(px)
        X.set_observed(ob)
    deep, keep = pc.thinner(P, 1e-3)
    signs = set()
    for k, atm in enumerate((P.atm, P.atm, deep, P.atm)):      # fresh, hinted, resuming deeper, hinted again
        spec_ref = plain.run(atm, P.opts)["spectrum"]
        pairs = E.run_pixels(atm, P.opts, SHIFTS)
        mom, spec = E.run_moments(atm, P.opts, SHIFTS, spectrum=True)
        assert np.array_equal(spec, spec_ref)
        for p in xc.OFF_GRID:
            assert np.all(pairs[:, p, 1] == 0)
        assert np.count_nonzero(pairs[..., 1] > 0) == 7 * 798
        ref = xc.check_moments(mom, pairs, ob, "%s run %d" % (solution, k))
        want_n = np.add.reduceat(((pairs[..., 1] > 0) & (ob.weight > 0)).astype(float), ob.seg_first[:-1][np.diff(ob.seg_first) > 0], axis=1)
        assert np.array_equal(mom[..., 0][:, np.diff(ob.seg_first) > 0], want_n)
        signs |= set(np.sign(ref[..., xcor.WFG]).ravel().tolist())
        # a handle that makes moments only goes through the same four states: the same bits
        assert np.array_equal(only.run_moments(atm, P.opts, SHIFTS), mom), k
    assert {-1.0, 1.0} <= signs
    # a segment with windows of both forms in it; no weights, no gain
    ob2 = xcor.Observed(xcor.segments([300, 200, 300]), ob.data)
    E.set_observed(ob2)
    mom = E.run_moments(P.atm, P.opts, SHIFTS)
    xc.check_moments(mom, E.run_pixels(P.atm, P.opts, SHIFTS), ob2, "%s [300, 200, 300], w = gain = 1" % solution)
    assert mom[0, :, 0].tolist() == [299.0, 200.0, 299.0] and np.array_equal(mom[..., 1], mom[..., 0])
    plain.close(); E.close(); only.close()


def test_bits_do_not_depend_on_the_rest_of_the_call(tmp_path):
    P = pc.make(tmp_path, "eclipse", nlines=20_000)
    px = xc.pixel_set(P)
    E = Engine(P.static)
    E.set_pixels(px)
    scale = float(np.mean(E.run(P.atm, P.opts)["spectrum"]))
    ob = xc.observed(len(px), scale)
    E.set_observed(ob)
    first = E.run_moments(P.atm, P.opts, SHIFTS)
    assert np.all(first[:, 5] == 0) and np.all(first[:, [1, 2, 3, 4, 7], 0] > 0)
    for _ in range(2):
        assert np.array_equal(E.run_moments(P.atm, P.opts, SHIFTS), first)
    assert np.array_equal(E.run_moments(P.atm, P.opts, SHIFTS, spectrum=True)[0], first)
    # the exposures permuted: the rows permute
    perm = [4, 0, 6, 2, 5, 1, 3]
    E.set_observed(xcor.Observed(ob.seg_first, ob.data[perm], ob.weight[perm], ob.gain))
    assert np.array_equal(E.run_moments(P.atm, P.opts, SHIFTS[perm]), first[perm])
    # the same pixels cut into other segments, more of them: a segment that keeps its pixels keeps its bits
    lengths = [1, 30, 33, 64, 65, 100, 100, 0, 0, 7, 150, 250]
    again = xcor.Observed(xcor.segments(lengths), ob.data, ob.weight, ob.gain)
    same = {0: 0, 3: 2, 4: 3, 7: 5, 8: 5, 9: 6}              # new segment -> the old one of the same pixels
    for new, old in same.items():
        assert again.seg_first[new:new + 2].tolist() == ob.seg_first[old:old + 2].tolist()
    E.set_observed(again)
    got = E.run_moments(P.atm, P.opts, SHIFTS)
    assert got.shape == (7, 12, 7)
    for new, old in same.items():
        assert np.array_equal(got[:, new], first[:, old]), (new, old)
    assert not np.array_equal(got[:, 1], first[:, 1])
    # another segment's data and weights changed: only that segment's rows change
    f, w = ob.data.copy(), ob.weight.copy()
    f[:, 193:393] *= -1.5
    w[:, 193:393] = 1.0
    E.set_observed(xcor.Observed(ob.seg_first, f, w, ob.gain))
    got = E.run_moments(P.atm, P.opts, SHIFTS)
    others = [0, 1, 2, 3, 5, 6, 7]
    assert np.array_equal(got[:, others], first[:, others])
    assert np.all(got[:, 4, 1:] != first[:, 4, 1:])
    E.close()


def test_chi_square_and_likelihood_end_to_end(tmp_path):
    P = pc.make(tmp_path, "transit", nlines=20_000)
    px = xc.pixel_set(P)
    E = Engine(P.static)
    E.set_pixels(px)
    scale = float(np.mean(E.run(P.atm, P.opts)["spectrum"]))
    ob = xc.observed(len(px), scale, seed=9)
    E.set_observed(ob)
    pairs = E.run_pixels(P.atm, P.opts, SHIFTS)
    mom = E.run_moments(P.atm, P.opts, SHIFTS)
    use = (pairs[..., 1] > 0) & (ob.weight > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = ob.gain[None, :] * pixels.value(pairs)
    f, w = ob.data, ob.weight
    tol = (max(xc.LENGTHS) + 32) * xc.EPS
    for a, b in ((1.0, 0.0), (0.8, 0.05 * scale)):
        got = xcor.chi2(mom, a, b)
        worst = 0.0
        for v in range(ob.nexp):
            for s in range(ob.nseg):
                k = np.arange(ob.seg_first[s], ob.seg_first[s + 1])
                k = k[use[v, k]]
                want = math.fsum(w[v, k] * (f[v, k] - a * g[v, k] - b) ** 2)
                size = math.fsum(w[v, k] * (np.abs(f[v, k]) + abs(a) * np.abs(g[v, k]) + abs(b)) ** 2)
                assert abs(got[v, s] - want) <= tol * size, (a, b, v, s, got[v, s], want)
                if size:
                    worst = max(worst, abs(got[v, s] - want) / size)
        print("chi2(a = %g, b = %g): worst error / sum of absolute terms %.3e (tolerance %.3e)" % (a, b, worst, tol))
        assert xcor.chi2_sum(mom, a, b) == pytest.approx(float(got.sum()), rel=1e-15)
    # the log-likelihood: finite wherever a segment has two pixels, and the direct value (means subtracted first)
    ll = xcor.loglike_bl19(mom)
    worst = 0.0
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
    print("loglike_bl19: worst relative difference from the direct value %.3e (tolerance 1e-10)" % worst)
    assert worst <= 1e-10
    assert math.isfinite(xcor.loglike_bl19_sum(mom)) and np.isnan(ll).sum() >= 2 * ob.nexp
    assert np.all(np.abs(xcor.ccf(mom)[~np.isnan(ll)]) <= 1.0)
    E.close()


def test_batch_moments_are_the_single_handle_moments(tmp_path):
    P = pc.make(tmp_path, "eclipse", nlines=30_000, seed=33)
    px = xc.pixel_set(P)
    K = 4
    atms, keep = pc.atmospheres(P, K)
    shifts = np.stack([np.roll(SHIFTS, j) * (1.0 + 1e-6 * j) for j in range(K)])
    one = Engine(P.static)
    one.set_pixels(px)
    ob = xc.observed(len(px), float(np.mean(one.run(P.atm, P.opts)["spectrum"])))
    one.set_observed(ob)
    ref = np.stack([one.run_moments(atms[j], P.opts, shifts[j]) for j in range(K)])
    one.close()
    assert len({ref[j].tobytes() for j in range(K)}) == K
    B = Batch(P.static, ways=3)
    B.set_pixels(px)
    B.set_observed(ob)
    for rep in range(2):
        got = B.run_moments(atms, P.opts, shifts)
        assert got.shape == (K, 7, 8, 7)
        assert np.array_equal(got, ref), rep
    B.close()


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
    for k in range(2):
        ref = plain.run(P.atm, P.opts)["spectrum"]
        pairs = E.run_pixels(P.atm, P.opts, shifts)
        mom, spec = E.run_moments(P.atm, P.opts, shifts, spectrum=True)
        assert np.array_equal(spec, ref)
        xc.check_moments(mom, pairs, ob, "opacity grid run %d" % k)
        assert np.array_equal(E.run(P.atm, P.opts)["spectrum"], ref)
    plain.close(); E.close()


def test_refusals_and_lifetimes(tmp_path):
    P = pc.make(tmp_path, "eclipse", nlines=10_000)
    sh = np.ascontiguousarray(SHIFTS[:3])
    good_px = pixels.Pixels([2510.0, 2520.0, 2530.0, 2540.0], [0.2, 0.3, 1.5, 0.4], 4.0)
    rng = np.random.default_rng(2)
    f, w, gain = rng.standard_normal((3, 4)), rng.uniform(0.5, 2.0, (3, 4)), rng.uniform(0.5, 1.5, 4)
    good = xcor.Observed([0, 1, 4], f, w, gain)
    E, bare = Engine(P.static), Engine(P.static)
    lib = E._lib
    dp = _abi.c_double_p
    with pytest.raises(EngineError) as ei:             # no pixel set to install it over
        E.set_observed(good)
    assert ei.value.code == -1 and "pixel set" in str(ei.value)
    E.set_pixels(good_px)
    bare.set_pixels(good_px)
    with pytest.raises(EngineError) as ei:             # no observed set
        E.run_moments(P.atm, P.opts, sh)
    assert ei.value.code == -1 and "observed" in str(ei.value)
    E.set_observed(good)
    before = E.run_moments(P.atm, P.opts, sh)
    assert before.shape == (3, 2, 7) and np.array_equal(before[..., 0], [[1, 3]] * 3)
    # run_pixels and run know nothing of the observed set
    assert np.array_equal(E.run_pixels(P.atm, P.opts, sh), bare.run_pixels(P.atm, P.opts, sh))
    assert np.array_equal(E.run(P.atm, P.opts)["spectrum"], bare.run(P.atm, P.opts)["spectrum"])

    def changed(**kw):
        args = dict(seg_first=[0, 1, 4], data=f.copy(), weight=w.copy(), gain=gain.copy())
        for k, (idx, val) in kw.items():
            args[k] = np.array(args[k], dtype=np.int64 if k == "seg_first" else np.float64)
            args[k][idx] = val
        return xcor.Observed(**args)

    bad = {
        "seg_first[0]": (changed(seg_first=(0, 1)), "seg_first"),
        "decreasing": (xcor.Observed([0, 3, 2, 4], f, w, gain), "seg_first"),
        "seg_first[nseg] short": (changed(seg_first=(2, 3)), "seg_first"),
        "seg_first[nseg] long": (changed(seg_first=(2, 5)), "seg_first"),
        "datum nan": (changed(data=((1, 2), np.nan)), "exposure 1 pixel 2"),
        "datum inf": (changed(data=((2, 0), np.inf)), "exposure 2 pixel 0"),
        "weight < 0": (changed(weight=((1, 2), -1.0)), "exposure 1 pixel 2"),
        "weight nan": (changed(weight=((0, 3), np.nan)), "exposure 0 pixel 3"),
        "weight inf": (changed(weight=((2, 1), np.inf)), "exposure 2 pixel 1"),
        "gain nan": (changed(gain=(3, np.nan)), "pixel 3"),
        "gain inf": (changed(gain=(0, -np.inf)), "pixel 0"),
    }
    for what, (ob, name) in bad.items():
        with pytest.raises(EngineError) as ei:
            E.set_observed(ob)
        assert ei.value.code == -1 and name in str(ei.value), (what, str(ei.value))
        assert np.array_equal(E.run_moments(P.atm, P.opts, sh), before), what
    assert "datum" in _refusal(E, bad["datum nan"][0]) and "weight" in _refusal(E, bad["weight < 0"][0])
    assert "gain" in _refusal(E, bad["gain nan"][0])

    def raw(**kw):
        c = good.to_c()
        for k, v in kw.items():
            setattr(c, k, v)
        return lib.trx_set_observed(E._h, C.byref(c)), lib.trx_last_error(E._h)

    assert raw(nexp=-1) == (-1, b"observed: nexp < 0")
    assert raw(nseg=0)[0] == -1 and raw(nseg=-2)[0] == -1 and b"nseg" in raw(nseg=0)[1]
    assert raw(seg_first=None)[0] == -1 and raw(data=None)[0] == -1 and b"NULL" in raw(data=None)[1]
    rc, msg = raw(nexp=2 ** 30)                        # 2^30 exposures x 2 segments: refused before the data are looked at
    assert rc == -1 and b"2^31" in msg
    assert np.array_equal(E.run_moments(P.atm, P.opts, sh), before)
    # the run's own refusals
    out = np.zeros_like(before)

    def run(nshift, shift, dest):
        return lib.trx_run_moments(E._h, C.byref(P.atm), C.byref(P.opts), None, nshift,
                                   shift.ctypes.data_as(dp) if shift is not None else None,
                                   dest.ctypes.data_as(dp) if dest is not None else None, None)

    assert run(2, sh, out) == -1 and b"nexp" in lib.trx_last_error(E._h)
    four = np.ascontiguousarray(SHIFTS[:4])
    assert run(4, four, np.zeros((4, 2, 7))) == -1 and run(0, sh, out) == -1
    assert run(3, None, out) == -1 and run(3, sh, None) == -1
    for what, v in (("nan", np.nan), ("inf", np.inf), ("0", 0.0), ("< 0", -1.0)):
        s = sh.copy()
        s[1] = v
        assert run(3, s, out) == -1, what
        assert b"shift 1 must be finite and > 0" in lib.trx_last_error(E._h), what
    assert np.all(out == 0)
    assert run(3, sh, out) == 0 and np.array_equal(out, before)
    # a refused set_pixels keeps both sets, a successful one drops the observed set
    with pytest.raises(EngineError):
        E.set_pixels(pixels.Pixels([2510.0, 2520.0, 2530.0, 2540.0], [0.2, 0.3, 0.0, 0.4], 4.0))
    assert np.array_equal(E.run_moments(P.atm, P.opts, sh), before)
    E.set_pixels(good_px)
    with pytest.raises(EngineError) as ei:
        E.run_moments(P.atm, P.opts, sh)
    assert ei.value.code == -1 and "observed" in str(ei.value)
    E.set_observed(good)
    assert np.array_equal(E.run_moments(P.atm, P.opts, sh), before)
    E.set_pixels(None)                                 # a clearing one too
    assert run(3, sh, out) == -1
    E.set_pixels(good_px)
    E.set_observed(good)
    E.set_observed(None)                               # cleared: refused again
    with pytest.raises(EngineError):
        E.run_moments(P.atm, P.opts, sh)
    assert np.array_equal(E.run_pixels(P.atm, P.opts, sh), bare.run_pixels(P.atm, P.opts, sh))
    E.close(); bare.close()
    # a shard's partial pairs say nothing about the moments
    n = P.nwn
    try:
        P.set_shard(1000, 3000)
        S = Engine(P.static)
        S.set_pixels(good_px)
        S.set_observed(good)
        with pytest.raises(EngineError) as ei:
            S.run_moments(P.atm, P.opts, sh)
        assert ei.value.code == -6 and "trx_run_pixels" in str(ei.value) and "trx_gather_host" in str(ei.value)
        assert S.run_pixels(P.atm, P.opts, sh).shape == (3, 4, 2)
        S.close()
    finally:
        P.set_shard(0, n)
    # a batch installs a set on every handle or on none
    B = Batch(P.static, ways=2)
    three = np.stack([sh] * 3)
    with pytest.raises(EngineError):
        B.set_observed(good)
    B.set_pixels(good_px)
    with pytest.raises(EngineError):
        B.run_moments([P.atm], P.opts, three[:1])
    B.set_observed(good)
    ref = B.run_moments([P.atm, P.atm, P.atm], P.opts, three)
    assert np.array_equal(ref[0], before) and np.array_equal(ref[2], before)
    with pytest.raises(EngineError) as ei:
        B.set_observed(bad["weight < 0"][0])
    assert "exposure 1 pixel 2" in str(ei.value)
    assert np.array_equal(B.run_moments([P.atm, P.atm, P.atm], P.opts, three), ref)
    with pytest.raises(EngineError) as ei:             # a bad shift of one atmosphere fails the call and names it
        worse = three.copy()
        worse[1, 2] = 0.0
        B.run_moments([P.atm, P.atm, P.atm], P.opts, worse)
    assert "shift 2" in str(ei.value)
    with pytest.raises(EngineError):                   # nshift != nexp
        B.run_moments([P.atm], P.opts, np.stack([SHIFTS[:2]]))
    B.set_pixels(good_px)                              # drops it on every handle
    with pytest.raises(EngineError):
        B.run_moments([P.atm], P.opts, three[:1])
    B.close()


def _refusal(E, ob):
    with pytest.raises(EngineError) as ei:
        E.set_observed(ob)
    return str(ei.value)
