"""The high-pass of the model pixels along each order on the device (trx_set_highpass / trx_run_highpassed /
trx_batch_set_highpass, include/transit_hip.h) against transit_amd.xcor.highpass_reference, the numpy statement of the
same definition: BIT EQUALITY, NaN in the same places.

The case is xcor_checks' with its straddling pixel: 6001 bins, 60 layers (20 000 lines where only bits are compared), the seven SHIFTS, the
800-pixel set with its two off-grid pixels and the straddling one, segment lengths [1, 63, 64, 65, 200, 0, 7, 400].  A
second pixel set has ONE segment of 2 kHpTile + 17 pixels: two full tiles and a ragged one, halos that cross tile borders
inside a segment, a dead pixel within `half` of a tile border.  Halves 0, 1, 5, 70 (wider than the 63, 64 and 65 pixel
segments), 450 (wider than every segment of the first set) and 1024 (the cap: the kernel's largest LDS tile).

Downstream the moments are held against xcor over the VALUES THE DEVICE RETURNED, by the rule of
xcor_checks.check_filtered_moments -- the count exact, every other moment to (n_max + 16) * 2^-52 of the sum of its absolute terms -- written
here as |mom - ref| <= tolerance * scale: a one-pixel segment's g' is exactly 0, its sums of absolute terms with it, and
such a row must then be exact (the quotient of that check's form is 0 / 0 there).  The filtered values by
xcor_checks.check_values; trail rows and maps against their own contracts, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import pixel_cases as pc
import xcor_checks as xc
from bits import same_bits
from transit_amd import _abi, broaden, pixels, xcor
from transit_amd.engine import Batch, Engine, EngineError

pytestmark = pytest.mark.gpu

SHIFTS = pc.SHIFTS
TILE = 512                                             # kHpTile
LONG = 2 * TILE + 17
LONG_DEAD = {TILE - 12: 2400.0, 2 * TILE + 3: 2700.0}   # pixel -> centre (cm-1), off the grid: 12 below a tile border, 3 above one


def check_sums(mom, ref, scale, ob, what=""):
    """moments [..., nseg, 7] against the reference's and the sums of its absolute terms: the count exactly, every other
    moment within (n_max + 16) * 2^-52 of the scale (exactly where the scale is 0), an empty row seven +0"""
    assert mom.shape == ref.shape == scale.shape
    assert np.array_equal(mom[..., 0], ref[..., 0]), what
    tol = (int(np.max(np.diff(ob.seg_first))) + 16) * xc.EPS
    empty = ref[..., 0] == 0
    assert np.any(empty) and np.all(mom[empty] == 0) and not np.any(np.signbit(mom[empty])), what
    err, size = np.abs(mom - ref)[..., 1:], scale[..., 1:]
    worst = float(np.max(err[size > 0] / size[size > 0]))
    print("%s: worst |mom - ref| / abs_ref %.3e = %.2f * 2^-52 (tolerance %.3e); %d sums of scale 0" % (what, worst, worst / xc.EPS, tol, np.count_nonzero(size == 0)))
    assert np.all(err <= tol * size), (what, worst, tol)


def check_moments(mom, val, ob, what=""):
    check_sums(mom, xcor.reference_values(val, ob), xcor.abs_reference_values(val, ob), ob, what)


def gain_free(ob):
    return xcor.Observed(ob.seg_first, ob.data, ob.weight, None)


def long_pixel_set(P):
    wn_d = float(P.static.wn_d)
    px = pixels.resolving_power(np.linspace(2503, 2557, LONG) + 0.37 * wn_d, 20000.0, 4.0)
    for p, c in LONG_DEAD.items():
        px.centre[p] = c
    return px


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """(P, px, ob): the eclipse case at 20 000 lines, the 800 pixels with the straddling one, the observed set"""
    P = pc.make(tmp_path_factory.mktemp("highpass"), "eclipse", nlines=20_000)
    px = xc.straddle_pixel_set(P)
    plain = Engine(P.static)
    scale = float(np.mean(plain.run(P.atm, P.opts)["spectrum"]))
    plain.close()
    return P, px, xc.observed(len(px), scale)


def handle(P, px, ob, hp=None):
    E = Engine(P.static)
    E.set_pixels(px)
    E.set_observed(ob)
    if hp is not None:
        E.set_highpass(hp)
    return E


# ---- 1. the values are the definition --------------------------------------------------------------------
@pytest.mark.parametrize("solution", ["eclipse", "transit"])
def test_values_are_the_definition_bit_for_bit(tmp_path, solution):
    P = pc.make(tmp_path, solution)
    assert P.nwn == 6001
    px = xc.straddle_pixel_set(P)
    plain = Engine(P.static)
    ob = xc.observed(len(px), float(np.mean(plain.run(P.atm, P.opts)["spectrum"])))
    E = handle(P, px, ob)
    deep, keep = pc.thinner(P, 1e-3)
    first = xc.highpass_tables(5)["gauss"]
    seen = set()
    for k, atm in enumerate((P.atm, P.atm, deep, P.atm)):      # fresh, hinted, resuming deeper, hinted again
        what = "%s run %d" % (solution, k)
        E.set_highpass(first)
        val, spec = E.run_highpassed(atm, P.opts, SHIFTS, spectrum=True)      # (the run that meets the handle in that state)
        assert np.array_equal(spec, plain.run(atm, P.opts)["spectrum"]), what
        pairs = E.run_pixels(atm, P.opts, SHIFTS)
        for p in xc.STRADDLE:                          # on the grid at exactly one shift: dead in six rows, live in one
            assert np.count_nonzero(pairs[:, p, 1] > 0) == 1 and pairs[0, p, 1] > 0
        assert same_bits(val, xcor.highpass_reference(pairs, ob, first)), what
        assert np.array_equal(np.isnan(val), ~(pairs[..., 1] > 0)), what
        assert np.flatnonzero(np.isnan(val).all(axis=0)).tolist() == sorted(xc.OFF_GRID), what
        for half in (0, 1, 5, 70, 450):
            for name, hp in xc.highpass_tables(half, seed=k).items():
                assert hp.half == half
                E.set_highpass(hp)
                got = E.run_highpassed(atm, P.opts, SHIFTS)
                ref = xcor.highpass_reference(pairs, ob, hp)
                assert same_bits(got, ref), (what, half, name, int(np.sum(got != ref)))
                if half == 0 and hp.taps[0] == 1.0:
                    live = ~np.isnan(got)
                    assert np.all(got[live] == 0) and not np.any(np.signbit(got[live])), (what, name)
        seen.add(val.tobytes())
    assert len(seen) == 2                              # the thinner atmosphere's values are other ones
    plain.close(); E.close()


@pytest.mark.parametrize("half", [5, 70, 450, 1024])
def test_one_long_segment_of_two_tiles_and_a_ragged_one(case, half):
    P = case[0]
    px = long_pixel_set(P)
    rng = np.random.default_rng(half)
    ob = xcor.Observed(xcor.segments([LONG]), rng.standard_normal((3, LONG)), None, rng.uniform(0.5, 1.5, LONG))
    E = handle(P, px, ob)
    shifts = SHIFTS[1:6]                                # (5 rows: not the set's 3 exposures)
    pairs = E.run_pixels(P.atm, P.opts, shifts)
    assert np.all(pairs[:, sorted(LONG_DEAD), 1] == 0) and np.count_nonzero(pairs[..., 1] > 0) == 5 * (LONG - 2)
    for name, hp in xc.highpass_tables(half).items():
        E.set_highpass(hp)
        got = E.run_highpassed(P.atm, P.opts, shifts)
        ref = xcor.highpass_reference(pairs, ob, hp)
        assert got.shape == (5, LONG) and same_bits(got, ref), (half, name, int(np.sum(got != ref)))
        assert np.flatnonzero(np.isnan(got).any(axis=0)).tolist() == sorted(LONG_DEAD)
    E.close()


# ---- 2. downstream -----------------------------------------------------------------------------------------
def test_moments_filter_trail_and_map_take_the_high_passed_model(case):
    P, px, ob = case
    hp = xc.highpass_tables(70)["gauss"]
    E = handle(P, px, ob, hp)
    val = E.run_highpassed(P.atm, P.opts, SHIFTS)
    dead = np.flatnonzero(np.isnan(val).any(axis=0)).tolist()
    assert dead == xc.DEAD
    # the moments of the values the device returned
    mom = E.run_moments(P.atm, P.opts, SHIFTS)
    check_moments(mom, val, ob, "high-passed moments")
    bare = handle(P, px, ob)
    assert not np.array_equal(mom, bare.run_moments(P.atm, P.opts, SHIFTS))
    # the filter behind the high-pass: the definition over the pairs (g', 1) / (0, 0), gains in them already
    F = xcor.svd_filter(ob.data, ob.seg_first, 3)
    E.set_filter(F)
    fmom, fval = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    xc.check_values(fval, xcor.highpass_pairs(val), gain_free(ob), F, "filter behind the high-pass")
    assert np.flatnonzero(np.isnan(fval).any(axis=0)).tolist() == dead and np.isnan(fval[:, dead]).all()
    check_moments(fmom, fval, ob, "filtered high-passed moments")
    assert np.array_equal(E.run_moments(P.atm, P.opts, SHIFTS), mom)      # (the filter is the filtered run's alone)
    # the trail: row l is run_moments with every shift equal to lag l, on the same handle
    lags = np.array([SHIFTS[1], SHIFTS[4], SHIFTS[1]])
    trail = E.run_trail(P.atm, P.opts, lags)
    for l, lag in enumerate(lags):
        assert np.array_equal(trail[l], E.run_moments(P.atm, P.opts, [lag] * ob.nexp)), l
    assert np.array_equal(trail[2], trail[0]) and not np.array_equal(trail[1], trail[0])
    assert not np.array_equal(trail, bare.run_trail(P.atm, P.opts, lags))
    # ... and the definition over the high-passed values of the lags' rows
    tval = E.run_highpassed(P.atm, P.opts, lags)
    tpairs = xcor.highpass_pairs(tval)
    check_sums(trail, xcor.trail_reference(tpairs, gain_free(ob)), xcor.trail_abs_reference(tpairs, gain_free(ob)), ob, "high-passed trail")
    # the map of its own per, bit for bit; per is the statistic of the high-passed trail
    vm = xc.the_map("ccf")
    m, per = E.run_velocity_map(P.atm, P.opts, vm, per=True)
    assert np.array_equal(m, xcor.map_from_per(per, vm), equal_nan=True)
    assert np.array_equal(np.isnan(m), xc.OUTSIDE)
    xc.check_per(per, E.run_trail(P.atm, P.opts, vm.lag), vm, "high-passed trail")
    assert not np.array_equal(per, bare.run_velocity_map(P.atm, P.opts, vm, per=True)[1])
    # half = 0, tap 1: g' is +0 at every live pixel -- the three moments with a factor g are +0 in every row
    E.set_highpass(xcor.boxcar_highpass(1))
    zero = E.run_moments(P.atm, P.opts, SHIFTS)
    for c in (xcor.WG, xcor.WGG, xcor.WFG):
        assert np.all(zero[..., c] == 0) and not np.any(np.signbit(zero[..., c])), c
    assert np.array_equal(zero[..., [xcor.N, xcor.W, xcor.WF, xcor.WFF]], mom[..., [xcor.N, xcor.W, xcor.WF, xcor.WFF]])
    E.close(); bare.close()


# ---- 3. independence -----------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_rest_of_the_call(case):
    P, px, ob = case
    hp = xc.highpass_tables(70)["random"]
    E = handle(P, px, ob, hp)
    val = E.run_highpassed(P.atm, P.opts, SHIFTS)
    for _ in range(2):
        assert same_bits(E.run_highpassed(P.atm, P.opts, SHIFTS), val)
    # rows added, permuted, alone
    perm = np.array([3, 0, 6, 2, 5, 1, 4])
    assert same_bits(E.run_highpassed(P.atm, P.opts, SHIFTS[perm]), val[perm])
    more = np.concatenate([SHIFTS[:2] * (1.0 + 1e-5), SHIFTS, SHIFTS[4:5]])
    got = E.run_highpassed(P.atm, P.opts, more)
    assert got.shape == (10, 800) and same_bits(got[2:9], val) and same_bits(got[9], val[4]) and not same_bits(got[0], val[0])
    assert same_bits(E.run_highpassed(P.atm, P.opts, SHIFTS[2:3]), val[2:3])
    mom = E.run_moments(P.atm, P.opts, SHIFTS)
    # the same pixels cut into other segments: a segment that keeps its pixels keeps its values and its rows; one that was
    # re-cut has other values within `half` of the new cut
    lengths = [1, 30, 33, 64, 65, 100, 100, 0, 0, 7, 150, 250]
    again = xcor.Observed(xcor.segments(lengths), ob.data, ob.weight, ob.gain)
    same = {0: 0, 3: 2, 4: 3, 7: 5, 8: 5, 9: 6}              # new segment -> the old one of the same pixels
    E.set_observed(again)
    E.set_highpass(hp)
    val2 = E.run_highpassed(P.atm, P.opts, SHIFTS)
    mom2 = E.run_moments(P.atm, P.opts, SHIFTS)
    assert mom2.shape == (7, 12, 7)
    for new, old in same.items():
        a, z = again.seg_first[new:new + 2]
        assert again.seg_first[new:new + 2].tolist() == ob.seg_first[old:old + 2].tolist()
        assert same_bits(val2[:, a:z], val[:, a:z]), (new, old)
        assert np.array_equal(mom2[:, new], mom[:, old]), (new, old)
    for new in (1, 2, 5, 6, 10, 11):
        a, z = again.seg_first[new:new + 2]
        live = ~np.isnan(val[0, a:z])
        assert np.any(val2[0, a:z][live] != val[0, a:z][live]), new
    # through a batch of two ways: each atmosphere's moments are the single handle's
    K = 3
    atms, keep = pc.atmospheres(P, K)
    shifts = np.stack([np.roll(SHIFTS, j) * (1.0 + 1e-6 * j) for j in range(K)])
    E.set_observed(ob)
    E.set_highpass(hp)
    ref = np.stack([E.run_moments(atms[j], P.opts, shifts[j]) for j in range(K)])
    E.set_highpass(None)
    plain = np.stack([E.run_moments(atms[j], P.opts, shifts[j]) for j in range(K)])
    assert len({ref[j].tobytes() for j in range(K)}) == K and not np.array_equal(ref, plain)
    E.close()
    B = Batch(P.static, ways=2)
    B.set_pixels(px)
    B.set_observed(ob)
    assert np.array_equal(B.run_moments(atms, P.opts, shifts), plain)
    B.set_highpass(hp)
    for rep in range(2):
        got = B.run_moments(atms, P.opts, shifts)
        assert got.shape == (K, 7, 8, 7) and np.array_equal(got, ref), rep
    B.set_highpass(None)
    assert np.array_equal(B.run_moments(atms, P.opts, shifts), plain)
    B.close()


# ---- 4. nobody else knows --------------------------------------------------------------------------------------
def test_the_other_runs_do_not_know_of_the_high_pass(case):
    P, px, ob = case
    E, bare = handle(P, px, ob, xc.highpass_tables(5)["boxcar"]), handle(P, px, ob)
    bs = pc.band_set(P)
    rot = broaden.Rotation.from_beta(1.037e-4)
    lags = SHIFTS[2:5]
    for X in (E, bare):
        X.set_bands(bs)
        X.set_broadening(rot)
    for k in range(2):
        E.run_highpassed(P.atm, P.opts, SHIFTS)
        E.run_moments(P.atm, P.opts, SHIFTS)
        assert np.array_equal(E.run(P.atm, P.opts)["spectrum"], bare.run(P.atm, P.opts)["spectrum"]), k
        assert np.array_equal(E.run_pixels(P.atm, P.opts, SHIFTS), bare.run_pixels(P.atm, P.opts, SHIFTS)), k
        assert np.array_equal(E.run_bands(P.atm, P.opts), bare.run_bands(P.atm, P.opts)), k
        assert np.array_equal(E.run_broadened(P.atm, P.opts), bare.run_broadened(P.atm, P.opts)), k
        assert not np.array_equal(E.run_moments(P.atm, P.opts, SHIFTS), bare.run_moments(P.atm, P.opts, SHIFTS)), k
    # the broadening is upstream of the high-pass: the values are the definition over the broadened pairs
    assert same_bits(E.run_highpassed(P.atm, P.opts, SHIFTS), xcor.highpass_reference(bare.run_pixels(P.atm, P.opts, SHIFTS), ob, xc.highpass_tables(5)["boxcar"]))
    # cleared: the parent's bits, those of a handle that never had one
    E.set_highpass(None)
    assert np.array_equal(E.run_moments(P.atm, P.opts, SHIFTS), bare.run_moments(P.atm, P.opts, SHIFTS))
    assert np.array_equal(E.run_trail(P.atm, P.opts, lags), bare.run_trail(P.atm, P.opts, lags))
    with pytest.raises(EngineError) as ei:
        E.run_highpassed(P.atm, P.opts, SHIFTS)
    assert ei.value.code == -1 and "high-pass" in str(ei.value)
    E.close(); bare.close()


# ---- 5. refusals and lifetimes ---------------------------------------------------------------------------------
def test_refusals_and_lifetimes(tmp_path):
    P = pc.make(tmp_path, "eclipse", nlines=10_000)
    sh = np.ascontiguousarray(SHIFTS[:3])
    good_px = pixels.Pixels([2510.0, 2520.0, 2530.0, 2540.0], [0.2, 0.3, 1.5, 0.4], 4.0)
    rng = np.random.default_rng(2)
    f, w, gain = rng.standard_normal((3, 4)), rng.uniform(0.5, 2.0, (3, 4)), rng.uniform(0.5, 1.5, 4)
    good_ob = xcor.Observed([0, 1, 4], f, w, gain)
    good = xcor.HighPass([1.0, 0.5, 0.25])
    E = Engine(P.static)
    lib = E._lib
    dp = _abi.c_double_p

    def refusal(X, hp):
        with pytest.raises(EngineError) as ei:
            X.set_highpass(hp)
        assert ei.value.code == -1
        return str(ei.value)

    assert "observed" in refusal(E, good)                              # no pixel set, no observed set
    E.set_pixels(good_px)
    assert "observed" in refusal(E, good)                              # no observed set to install it over
    E.set_observed(good_ob)
    with pytest.raises(EngineError) as ei:                             # no high-pass
        E.run_highpassed(P.atm, P.opts, sh)
    assert ei.value.code == -1 and "no high-pass installed" in str(ei.value)
    E.set_highpass(good)
    before = E.run_highpassed(P.atm, P.opts, sh)
    assert before.shape == (3, 4) and not np.isnan(before).any() and np.all(before[:, 0] == 0)      # (a segment of one pixel)
    mbefore = E.run_moments(P.atm, P.opts, sh)

    def unchanged(what):
        assert np.array_equal(E.run_highpassed(P.atm, P.opts, sh), before), what
        assert np.array_equal(E.run_moments(P.atm, P.opts, sh), mbefore), what

    for what, taps, name in (("nan", [1.0, np.nan], "tap 1"), ("inf", [1.0, 1.0, np.inf], "tap 2"), ("negative", [1.0, -0.5], "tap 1"),
                             ("tap 0 nan", [np.nan, 1.0], "tap 0"), ("tap 0 zero", [0.0, 1.0], "tap 0 must be > 0"),
                             ("too wide", np.ones(_abi.HIGHPASS_MAX_HALF + 2), "TRX_HIGHPASS_MAX_HALF (1024)")):
        assert name in refusal(E, xcor.HighPass(taps)), what
        unchanged(what)
    E.set_highpass(xcor.HighPass(np.ones(_abi.HIGHPASS_MAX_HALF + 1)))      # the cap itself is taken
    assert np.all(E.run_highpassed(P.atm, P.opts, sh)[:, 0] == 0)
    E.set_highpass(good)

    def raw(**kw):
        c = good.to_c()
        for k, v in kw.items():
            setattr(c, k, v)
        return lib.trx_set_highpass(E._h, C.byref(c)), lib.trx_last_error(E._h)

    assert raw(half=-1) == (-1, b"highpass: half < 0")
    assert raw(half=1025)[0] == -1 and b"TRX_HIGHPASS_MAX_HALF" in raw(half=1025)[1]
    unchanged("raw refusals")
    # the run's own refusals, all on the host
    out = np.zeros_like(before)

    def run(nshift, shift, dest):
        return lib.trx_run_highpassed(E._h, C.byref(P.atm), C.byref(P.opts), None, nshift,
                                      shift.ctypes.data_as(dp) if shift is not None else None,
                                      dest.ctypes.data_as(dp) if dest is not None else None, None)

    assert run(0, sh, out) == -1 and b"nshift < 1" in lib.trx_last_error(E._h)
    assert run(-2, sh, out) == -1
    assert run(3, None, out) == -1 and b"shift is NULL" in lib.trx_last_error(E._h)
    assert run(3, sh, None) == -1 and b"values is NULL" in lib.trx_last_error(E._h)
    for what, v in (("nan", np.nan), ("inf", np.inf), ("0", 0.0), ("< 0", -1.0)):
        s = sh.copy()
        s[1] = v
        assert run(3, s, out) == -1, what
        assert b"shift 1 must be finite and > 0" in lib.trx_last_error(E._h), what
    assert np.all(out == 0)
    assert run(3, sh, out) == 0 and np.array_equal(out, before)
    two = np.zeros((2, 4))
    assert run(2, sh, two) == 0 and np.array_equal(two, before[:2])      # any number of rows
    # a refused set_observed or set_pixels keeps the high-pass; a successful set_observed drops it, a clearing one too
    with pytest.raises(EngineError):
        E.set_observed(xcor.Observed([0, 3, 2, 4], f, w, gain))
    with pytest.raises(EngineError):
        E.set_pixels(pixels.Pixels([2510.0, 2520.0, 2530.0, 2540.0], [0.2, 0.3, 0.0, 0.4], 4.0))
    unchanged("refused sets")
    plain = Engine(P.static)
    plain.set_pixels(good_px)
    plain.set_observed(good_ob)
    mplain = plain.run_moments(P.atm, P.opts, sh)
    plain.close()
    assert not np.array_equal(mplain, mbefore)
    E.set_observed(good_ob)
    assert run(3, sh, out) == -1 and b"no high-pass installed" in lib.trx_last_error(E._h)
    assert np.array_equal(E.run_moments(P.atm, P.opts, sh), mplain)
    E.set_highpass(good)
    unchanged("installed again")
    E.set_observed(None)
    assert run(3, sh, out) == -1 and b"observed" in lib.trx_last_error(E._h) and "observed" in refusal(E, good)
    E.set_observed(good_ob)
    E.set_highpass(good)
    E.set_pixels(good_px)                              # drops both
    assert run(3, sh, out) == -1 and b"observed" in lib.trx_last_error(E._h)
    E.set_observed(good_ob)
    assert run(3, sh, out) == -1 and b"no high-pass installed" in lib.trx_last_error(E._h)
    E.set_highpass(good)
    unchanged("after set_pixels")
    # independent of the filter: installing or clearing one keeps the high-pass
    E.set_filter(xc.random_filter(2, 2, 3, seed=6))
    unchanged("with a filter")
    E.set_filter(None)
    unchanged("filter cleared")
    E.set_highpass(None)                               # cleared: refused again; taps NULL clears too
    assert run(3, sh, out) == -1
    E.set_highpass(good)
    assert raw(taps=None)[0] == 0 and run(3, sh, out) == -1 and b"no high-pass installed" in lib.trx_last_error(E._h)
    E.close()
    # a shard's partial pairs say nothing about the high-passed values
    n = P.nwn
    try:
        P.set_shard(1000, 3000)
        S = Engine(P.static)
        S.set_pixels(good_px)
        S.set_observed(good_ob)
        S.set_highpass(good)
        with pytest.raises(EngineError) as ei:
            S.run_highpassed(P.atm, P.opts, sh)
        assert ei.value.code == -6 and "trx_run_pixels" in str(ei.value)
        assert S.run_pixels(P.atm, P.opts, sh).shape == (3, 4, 2)
        S.close()
    finally:
        P.set_shard(0, n)
    # a batch installs a high-pass on every handle or on none
    B = Batch(P.static, ways=2)
    three = np.stack([sh] * 3)
    assert "observed" in refusal(B, good)
    B.set_pixels(good_px)
    B.set_observed(good_ob)
    assert np.array_equal(B.run_moments([P.atm, P.atm, P.atm], P.opts, three)[1], mplain)
    B.set_highpass(good)
    ref = B.run_moments([P.atm, P.atm, P.atm], P.opts, three)
    assert np.array_equal(ref[0], mbefore) and np.array_equal(ref[2], mbefore)
    assert "tap 1" in refusal(B, xcor.HighPass([1.0, np.nan]))
    assert np.array_equal(B.run_moments([P.atm, P.atm, P.atm], P.opts, three), ref)
    B.set_observed(good_ob)                            # drops it on every handle
    assert np.array_equal(B.run_moments([P.atm, P.atm, P.atm], P.opts, three)[2], mplain)
    B.close()
