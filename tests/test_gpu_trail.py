"""The cross-correlation trail on the device (trx_run_trail / trx_run_batch_trail, include/transit_hip.h): every
exposure of the observed set against the model at every lag of a grid.

The case is xcor_checks': pixel_cases.make (20 000-40 000 lines, 6001 bins, 60 layers), its 800-pixel set with the two
off-grid pixels, observed() with segment lengths [1, 63, 64, 65, 200, 0, 7, 400], 7 exposures, 5 % zero weights.  The
lags are its seven SHIFTS followed by the first two again, 9 in all: ragged for a lag tile of 2 or 4 (the last tile has
one lag), as the 7 exposures are for a tile of 4, and lags 7 and 8 repeat lags 0 and 1.

THE CONTRACT: trail[l] is, bit for bit, what run_moments gives on the same handle when all seven shifts equal lag l.

Tolerance of the accuracy check, per moment, relative to xcor.trail_abs_reference: (n_max + 16) * 2^-52 with n_max = 400
the longest segment -- the bound xcor_checks' docstring derives for the same sum in the same order (a double sum of n terms,
(n - 1) * 2^-53 each way it is ordered, each term of at most four correctly rounded operations); the count is exact.

The end-to-end test: the data are the model's own pixel values at the shifts of a planet with (Kp, Vsys) = (100, 6) km/s
over 7 phases in [-0.06, 0.06], times the gain, with unit weights; the lag grid is -81 .. 81 km/s in steps of 3 km/s --
the narrowest pixels (R = 20 000) have a FWHM of 15 km/s, a quarter of which is 3.75 -- and the map is 5 x 5 cells,
Kp = 40 .. 160 in steps of 30 and Vsys = -12 .. 12 in steps of 6, whose velocities all lie inside the lag grid
(|v| <= 12 + 160 sin(2 pi 0.06) = 70.9).  That numpy alone (pixels.reference over a CPU spectrum of this case, then
xcor.trail_reference, then velocity_map) puts the peak of this map at the injected cell (2, 3) was confirmed on the CPU
before the device was asked: 13.995 of the 14 that seven exposures x two segments can give there, against at most 13.872
anywhere else (the neighbours in Vsys 13.872 and 13.869, in Kp 13.829 and 13.830; the spectrum's broad shape correlates
at every lag, so the map is flat to a few percent -- and the peak stands 0.12 above it, ten orders over rounding)."""
import ctypes as C

import numpy as np
import pytest

import pixel_cases as pc
import xcor_checks as xc
from transit_amd import _abi, broaden, pixels, xcor
from transit_amd.engine import Batch, Engine, EngineError

pytestmark = pytest.mark.gpu

SHIFTS = pc.SHIFTS
LAGS = np.concatenate([SHIFTS, SHIFTS[:2]])


def by_moments(E, atm, opts, lags):
    """the trail by its contract: run_moments with every shift equal to the lag, lag by lag"""
    return np.stack([E.run_moments(atm, opts, [lag] * E.mom_shape[0]) for lag in lags])


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """(P, px, ob): the eclipse case at 20 000 lines, the 800 pixels, the observed set"""
    P = pc.make(tmp_path_factory.mktemp("trail"), "eclipse", nlines=20_000)
    px = xc.pixel_set(P)
    plain = Engine(P.static)
    scale = float(np.mean(plain.run(P.atm, P.opts)["spectrum"]))
    plain.close()
    return P, px, xc.observed(len(px), scale)


@pytest.mark.parametrize("solution", ["eclipse", "transit"])
def test_trail_is_the_moments_of_every_lag_bit_for_bit(tmp_path, solution):
    P = pc.make(tmp_path, solution)
    assert P.nwn == 6001
    px = xc.pixel_set(P)
    plain = Engine(P.static)
    ob = xc.observed(len(px), float(np.mean(plain.run(P.atm, P.opts)["spectrum"])))
    assert (ob.nexp, ob.nseg) == (7, 8)
    E = xc.handle(P, px, ob)
    deep, keep = pc.thinner(P, 1e-3)
    seen = set()
    for k, atm in enumerate((P.atm, P.atm, deep, P.atm)):      # fresh, hinted, resuming deeper, hinted again
        trail, spec = E.run_trail(atm, P.opts, LAGS, spectrum=True)
        assert trail.shape == (9, 7, 8, 7)
        assert np.array_equal(spec, plain.run(atm, P.opts)["spectrum"]), k
        want = by_moments(E, atm, P.opts, LAGS)
        for l in range(len(LAGS)):
            assert np.array_equal(trail[l], want[l]), (solution, k, l)
        assert np.array_equal(trail[7:], trail[:2])            # repeated lags, repeated rows
        assert len({trail[l].tobytes() for l in range(7)}) == 7
        assert np.array_equal(E.run_trail(atm, P.opts, LAGS), trail), k
        seen.add(trail.tobytes())
    assert len(seen) == 2                                      # the thinner atmosphere's trail is another one
    plain.close(); E.close()


def test_trail_is_the_definition_over_the_pixel_pairs(case):
    P, px, ob = case
    E = xc.handle(P, px, ob)
    assert np.count_nonzero(ob.weight == 0) > 100
    pairs = E.run_pixels(P.atm, P.opts, LAGS)
    trail = E.run_trail(P.atm, P.opts, LAGS)
    for p in xc.OFF_GRID:                                      # the off-grid pixels count nowhere
        assert np.all(pairs[:, p, 1] == 0)
    assert np.count_nonzero(pairs[..., 1] > 0) == 9 * 798
    ref = xc.check_trail(trail, pairs, ob, "9 lags x 7 exposures x 8 segments")
    some = np.diff(ob.seg_first) > 0
    want_n = np.add.reduceat(((pairs[:, None, :, 1] > 0) & (ob.weight[None] > 0)).astype(float), ob.seg_first[:-1][some], axis=2)
    assert np.array_equal(trail[..., 0][:, :, some], want_n)
    assert np.all(trail[:, :, 5] == 0) and not np.any(np.signbit(trail[:, :, 5]))      # the empty segment: seven +0
    assert {-1.0, 1.0} <= set(np.sign(ref[..., xcor.WFG]).ravel().tolist())
    E.close()


def test_bits_do_not_depend_on_the_rest_of_the_call(case):
    P, px, ob = case
    E = xc.handle(P, px, ob)
    first = E.run_trail(P.atm, P.opts, LAGS)
    # one lag; a permuted subset of the lags
    for l in (0, 4, 8):
        one = E.run_trail(P.atm, P.opts, LAGS[l:l + 1])
        assert one.shape == (1, 7, 8, 7) and np.array_equal(one[0], first[l]), l
    perm = [6, 2, 8, 3, 0]
    assert np.array_equal(E.run_trail(P.atm, P.opts, LAGS[perm]), first[perm])
    # another segment's data and weights changed: only that segment's rows change
    f, w = ob.data.copy(), ob.weight.copy()
    f[:, 193:393] *= -1.5
    w[:, 193:393] = 1.0
    E.set_observed(xcor.Observed(ob.seg_first, f, w, ob.gain))
    got = E.run_trail(P.atm, P.opts, LAGS)
    others = [0, 1, 2, 3, 5, 6, 7]
    assert np.array_equal(got[:, :, others], first[:, :, others])
    assert np.all(got[:, :, 4, 1:] != first[:, :, 4, 1:])
    # a segment with windows of both forms in it; no weights, no gain
    ob2 = xcor.Observed(xcor.segments([300, 200, 300]), ob.data)
    E.set_observed(ob2)
    trail = E.run_trail(P.atm, P.opts, LAGS)
    xc.check_trail(trail, E.run_pixels(P.atm, P.opts, LAGS), ob2, "[300, 200, 300], w = gain = 1")
    assert trail[0, 0, :, 0].tolist() == [299.0, 200.0, 299.0] and np.array_equal(trail[..., 1], trail[..., 0])
    assert np.array_equal(trail, by_moments(E, P.atm, P.opts, LAGS))
    E.close()


def test_broadening_applies_and_the_filter_does_not(case):
    P, px, ob = case
    E = xc.handle(P, px, ob)
    bare = E.run_trail(P.atm, P.opts, LAGS)
    # what the neighbours give before any trail with the other sets installed
    F = xcor.svd_filter(ob.data, ob.seg_first, 2)
    E.set_filter(F)
    before = (E.run_moments(P.atm, P.opts, SHIFTS), E.run_filtered_moments(P.atm, P.opts, SHIFTS), E.run_pixels(P.atm, P.opts, SHIFTS))
    # with a filter installed: the trail without it
    assert np.array_equal(E.run_trail(P.atm, P.opts, LAGS), bare)
    # the trail's larger pair buffer does not disturb the neighbours
    after = (E.run_moments(P.atm, P.opts, SHIFTS), E.run_filtered_moments(P.atm, P.opts, SHIFTS), E.run_pixels(P.atm, P.opts, SHIFTS))
    for a, b in zip(before, after):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(before[0], np.stack([bare[v, v] for v in range(xc.NEXP)]))      # the trail's diagonal IS the moment run
    # with a broadening installed: the contract, against run_moments under the same broadening
    E.set_broadening(broaden.Rotation(4.0, 0.4))
    broad = E.run_trail(P.atm, P.opts, LAGS)
    assert np.array_equal(broad, by_moments(E, P.atm, P.opts, LAGS))
    assert np.array_equal(broad[..., 0], bare[..., 0]) and np.all(broad[:, :, 7, 2] != bare[:, :, 7, 2])
    E.set_broadening(None)
    E.set_filter(None)
    assert np.array_equal(E.run_trail(P.atm, P.opts, LAGS), bare)
    E.close()


def test_batch_trails_are_the_single_handle_trails(tmp_path):
    P = pc.make(tmp_path, "eclipse", nlines=30_000, seed=33)
    px = xc.pixel_set(P)
    K = 3
    atms, keep = pc.atmospheres(P, K)
    lags = np.stack([np.roll(LAGS, j) * (1.0 + 1e-6 * j) for j in range(K)])
    one = Engine(P.static)
    one.set_pixels(px)
    ob = xc.observed(len(px), float(np.mean(one.run(P.atm, P.opts)["spectrum"])))
    one.set_observed(ob)
    ref = np.stack([one.run_trail(atms[j], P.opts, lags[j]) for j in range(K)])
    one.close()
    assert len({ref[j].tobytes() for j in range(K)}) == K
    B = Batch(P.static, ways=2)
    B.set_pixels(px)
    B.set_observed(ob)
    for rep in range(2):
        got = B.run_trail(atms, P.opts, lags)
        assert got.shape == (K, 9, 7, 8, 7)
        assert np.array_equal(got, ref), rep
    B.close()


def test_velocity_map_of_the_models_own_data_peaks_at_the_injected_cell(case):
    P, px, _ = case
    E = Engine(P.static)
    E.set_pixels(px)

    def trail_of(lags, ob):
        E.set_observed(ob)
        return E.run_trail(P.atm, P.opts, lags)

    m, cell = xc.end_to_end_map(px, lambda sh: E.run_pixels(P.atm, P.opts, sh), trail_of)
    peak = tuple(int(i) for i in np.unravel_index(np.argmax(m), m.shape))
    print("map (rows Kp, columns Vsys):\n%s\npeak at %s, injected at %s" % (np.array2string(m, precision=4), peak, cell))
    assert cell == (2, 3) and peak == cell
    assert m[cell] <= 2 * xc.NEXP * (1 + 1e-12)                   # a correlation coefficient per exposure and segment
    E.close()


def test_refusals(tmp_path):
    P = pc.make(tmp_path, "eclipse", nlines=10_000)
    lag = np.ascontiguousarray(LAGS[:5])
    good_px = pixels.Pixels([2510.0, 2520.0, 2530.0, 2540.0], [0.2, 0.3, 1.5, 0.4], 4.0)
    rng = np.random.default_rng(2)
    good = xcor.Observed([0, 1, 4], rng.standard_normal((3, 4)), rng.uniform(0.5, 2.0, (3, 4)), rng.uniform(0.5, 1.5, 4))
    E = Engine(P.static)
    lib, dp = E._lib, _abi.c_double_p
    with pytest.raises(EngineError) as ei:                     # no pixel set, no observed set
        E.run_trail(P.atm, P.opts, lag)
    assert ei.value.code == -1 and "observed" in str(ei.value)
    E.set_pixels(good_px)
    with pytest.raises(EngineError) as ei:
        E.run_trail(P.atm, P.opts, lag)
    assert ei.value.code == -1 and "observed" in str(ei.value)
    E.set_observed(good)
    before = E.run_trail(P.atm, P.opts, lag)
    assert before.shape == (5, 3, 2, 7) and np.array_equal(before[..., 0], np.broadcast_to([1.0, 3.0], (5, 3, 2)))
    out = np.zeros_like(before)

    def run(nlag, lags, dest):
        rc = lib.trx_run_trail(E._h, C.byref(P.atm), C.byref(P.opts), None, nlag,
                               lags.ctypes.data_as(dp) if lags is not None else None,
                               dest.ctypes.data_as(dp) if dest is not None else None, None)
        return rc, lib.trx_last_error(E._h)

    assert run(0, lag, out) == (-1, b"trx_run_trail: nlag < 1") and run(-3, lag, out)[0] == -1
    assert run(5, None, out) == (-1, b"trx_run_trail: lag is NULL")
    assert run(5, lag, None) == (-1, b"trx_run_trail: trail is NULL")
    for what, v in (("nan", np.nan), ("inf", np.inf), ("0", 0.0), ("< 0", -1.0)):
        s = lag.copy()
        s[1] = v
        rc, msg = run(5, s, out)
        assert rc == -1 and b"lag 1 must be finite and > 0" in msg, (what, msg)
    # 2^30 lags x 3 exposures x 2 segments: refused on the counts, before the lags are looked at
    rc, msg = run(2 ** 30, lag, out)
    assert rc == -1 and b"nlag * nexp * nseg above 2^31 - 1" in msg
    assert np.all(out == 0)
    # a refused run leaves the handle usable and the next trail's bits unchanged
    assert run(5, lag, out)[0] == 0 and np.array_equal(out, before)
    assert np.array_equal(E.run_trail(P.atm, P.opts, lag), before)
    # 2^31 - 1 lags x 800 pixels: more pairs than one pixel launch takes (one exposure, one segment: the rows fit)
    px = xc.pixel_set(P)
    E.set_pixels(px)
    E.set_observed(xcor.Observed([0, 800], np.zeros((1, 800))))
    rc, msg = run(2 ** 31 - 1, lag, out)
    assert rc == -1 and b"nlag * npix above what one pixel launch takes" in msg
    assert E.run_trail(P.atm, P.opts, lag).shape == (5, 1, 1, 7)
    E.close()
    # a shard's partial pairs say nothing about the moments
    n = P.nwn
    try:
        P.set_shard(1000, 3000)
        S = Engine(P.static)
        S.set_pixels(good_px)
        S.set_observed(good)
        with pytest.raises(EngineError) as ei:
            S.run_trail(P.atm, P.opts, lag)
        assert ei.value.code == -6 and "trx_run_pixels" in str(ei.value) and "trx_gather_host" in str(ei.value)
        assert S.run_pixels(P.atm, P.opts, lag).shape == (5, 4, 2)
        S.close()
    finally:
        P.set_shard(0, n)
    # the batch form
    B = Batch(P.static, ways=2)
    two = np.stack([lag, lag[::-1]])
    B.set_pixels(good_px)
    with pytest.raises(EngineError) as ei:                     # no observed set
        B.run_trail([P.atm, P.atm], P.opts, two)
    assert ei.value.code == -1 and "observed" in str(ei.value)
    B.set_observed(good)
    ref = B.run_trail([P.atm, P.atm], P.opts, two)
    assert np.array_equal(ref[0], before) and np.array_equal(ref[1], before[::-1])
    with pytest.raises(EngineError) as ei:                     # a bad lag of one atmosphere fails the call and names it
        worse = two.copy()
        worse[1, 2] = 0.0
        B.run_trail([P.atm, P.atm], P.opts, worse)
    assert "lag 2" in str(ei.value) and "atmosphere 1" in str(ei.value)
    with pytest.raises(EngineError) as ei:
        B.run_trail([P.atm, P.atm], P.opts, two[:, :0])
    assert "nlag < 1" in str(ei.value)
    assert np.array_equal(B.run_trail([P.atm, P.atm], P.opts, two), ref)
    B.close()
