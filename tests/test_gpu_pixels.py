"""Detector pixels at Doppler shifts on the device (trx_set_pixels / trx_run_pixels and the batch forms,
include/transit_hip.h).

A pixel run must leave the spectrum exactly as trx_run computes it and return, per shift and pixel, the pair of the
equivalent GAUSS band: checked against pixels.reference (math.fsum over the returned spectrum, the header's range rule)
and against trx_run_bands with pixels.as_bands on a second handle; for bit independence (repeats, with and without the
spectrum, inside a larger set, subsets and permutations of the shifts, through a batch); over shards; on an
opacity-grid handle; and for its refusals.

Tolerance of the two accuracy checks, per component, relative: pixel_cases.tolerance, 1e-12 + 2 * 2^-52 * nu_max / sigma_min,
derived in that module's docstring."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import pixel_cases as pc
from cases import GOLDEN
from transit_amd import _abi, bands, pixels
from transit_amd.engine import Batch, Engine, EngineError
from transit_amd.host import Problem

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("solution", ["eclipse", "transit"])
def test_pixel_runs_keep_the_spectrum_and_match_the_bands(tmp_path, solution):
    P = pc.make(tmp_path, solution)
    assert P.nwn == 6001
    A, B = pc.set_a(P), pc.set_b(P)
    la, ma = pc.window_lengths_and_margin(P, A, pc.SHIFTS)
    lb, mb = pc.window_lengths_and_margin(P, B, pc.SHIFTS)
    assert 42 <= la.min() and la.max() <= 44 and 283 <= lb.min() and lb.max() <= 290
    assert min(ma, mb) >= 1e-6, (ma, mb)
    px = pc.joined(A, B)
    tol = pc.tolerance(px, pc.SHIFTS)
    assert 1.5e-11 < tol < 3e-11
    plain, pix, banded = Engine(P.static), Engine(P.static), Engine(P.static)
    pix.set_pixels(px)
    banded.set_bands(pixels.as_bands(px, pc.SHIFTS))
    deep, keep = pc.thinner(P, 1e-3)
    for k, atm in enumerate((P.atm, P.atm, deep, P.atm)):      # fresh, hinted, resuming deeper, hinted again
        ref = plain.run(atm, P.opts)["spectrum"]
        out, spec = pix.run_pixels(atm, P.opts, pc.SHIFTS, spectrum=True)
        assert out.shape == (len(pc.SHIFTS), len(px), 2)
        assert np.array_equal(spec, ref)
        pc.check_accuracy(P, px, pc.SHIFTS, out, spec, tol, what="%s run %d vs reference" % (solution, k))
        sums = banded.run_bands(atm, P.opts).reshape(out.shape)
        pc.check_close(out, sums, tol, "%s run %d vs run_bands" % (solution, k))
        assert np.all(out[..., 1] > 0)
    # trx_run on a handle with pixels installed: the plain spectrum
    for atm in (P.atm, deep):
        assert np.array_equal(pix.run(atm, P.opts)["spectrum"], plain.run(atm, P.opts)["spectrum"])
    plain.close(); pix.close(); banded.close()


def test_one_bin_window_is_the_spectrum_value(tmp_path):
    P = pc.make(tmp_path, "eclipse", nlines=10_000)
    wn_i, wn_d, n, wn = pc.grid(P)
    px = pixels.Pixels([float(wn[n // 2])], [wn_d / 2], 1.0)
    assert bands.gauss_range(wn_i, wn_d, n, float(wn[n // 2]), wn_d / 2, 1.0) == (n // 2, n // 2 + 1)
    E = Engine(P.static)
    E.set_pixels(px)
    out, spec = E.run_pixels(P.atm, P.opts, [1.0], spectrum=True)
    assert out.shape == (1, 1, 2)
    assert out[0, 0, 0] == spec[n // 2] and out[0, 0, 1] == 1.0
    E.close()


def test_bits_do_not_depend_on_the_rest_of_the_call(tmp_path):
    P = pc.make(tmp_path, "eclipse", nlines=20_000)
    px = pc.joined(pc.set_a(P), pc.set_b(P))
    E = Engine(P.static)
    E.set_pixels(px)
    first = E.run_pixels(P.atm, P.opts, pc.SHIFTS)
    for _ in range(2):
        assert np.array_equal(E.run_pixels(P.atm, P.opts, pc.SHIFTS), first)
    assert np.array_equal(E.run_pixels(P.atm, P.opts, pc.SHIFTS, spectrum=True)[0], first)
    # subsets and a permutation of the shifts
    for idx in ([3], [0, 6], [5, 2, 4], [6, 5, 4, 3, 2, 1, 0], [1, 1, 0]):
        got = E.run_pixels(P.atm, P.opts, pc.SHIFTS[idx])
        assert np.array_equal(got, first[idx]), idx
    # the set between 300 other pixels (every lane and wave now holds other pairs)
    rng = np.random.default_rng(5)
    front = pixels.resolving_power(rng.uniform(2501, 2559, 137), 9000.0)
    back = pixels.resolving_power(rng.uniform(2490, 2570, 163), 2000.0)
    E.set_pixels(pc.joined(front, px, back))
    got = E.run_pixels(P.atm, P.opts, pc.SHIFTS)
    assert got.shape == (len(pc.SHIFTS), len(px) + 300, 2)
    assert np.array_equal(got[:, 137:137 + len(px)], first)
    E.close()


def test_batch_pairs_are_the_single_handle_pairs(tmp_path):
    P = pc.make(tmp_path, "eclipse", nlines=30_000, seed=33)
    px = pc.joined(pc.set_a(P), pc.set_b(P))
    K = 7
    atms, keep = pc.atmospheres(P, K)
    shifts = np.stack([np.roll(pc.SHIFTS, j)[:5] * (1.0 + 1e-6 * j) for j in range(K)])
    one = Engine(P.static)
    one.set_pixels(px)
    ref = np.stack([one.run_pixels(atms[j], P.opts, shifts[j]) for j in range(K)])
    one.close()
    assert len({ref[j].tobytes() for j in range(K)}) == K
    B = Batch(P.static, ways=3)
    B.set_pixels(px)
    for rep in range(2):
        got = B.run_pixels(atms, P.opts, shifts)
        assert got.shape == (K, 5, len(px), 2)
        assert np.array_equal(got, ref), rep
    B.close()


@pytest.mark.parametrize("solution", ["eclipse", "transit"])
def test_shards_combined_in_rank_order(tmp_path, solution):
    P = pc.make(tmp_path, solution, nlines=20_000)
    px = pc.joined(pc.set_a(P), pc.set_b(P))
    tol = pc.tolerance(px, pc.SHIFTS)
    wn_i, wn_d, n, _ = pc.grid(P)
    whole = Engine(P.static)
    whole.set_pixels(px)
    total, spec = whole.run_pixels(P.atm, P.opts, pc.SHIFTS, spectrum=True)
    whole.close()
    pc.check_accuracy(P, px, pc.SHIFTS, total, spec, tol, what="whole grid")
    ranges = [bands.gauss_range(wn_i, wn_d, n, b.centre, b.fwhm, b.cut) for b in pixels.as_bands(px, pc.SHIFTS)]
    cuts = [0, 1500, 3777, n]
    parts, empties = [], 0
    try:
        for r in range(3):
            P.set_shard(cuts[r], cuts[r + 1])
            E = Engine(P.static)
            E.set_pixels(px)
            s, sp = E.run_pixels(P.atm, P.opts, pc.SHIFTS, spectrum=True)
            E.close()
            assert sp.shape == (cuts[r + 1] - cuts[r],)
            pc.check_accuracy(P, px, pc.SHIFTS, s, sp, tol, lo=cuts[r], what="shard %d" % r)
            flat = s.reshape(-1, 2)
            for k, (a, z) in enumerate(ranges):
                if max(a, cuts[r]) >= min(z, cuts[r + 1]):
                    empties += 1
                    assert flat[k, 0] == 0 and flat[k, 1] == 0 and not np.signbit(flat[k, 0]) and not np.signbit(flat[k, 1]), (r, k)
            parts.append(s)
    finally:
        P.set_shard(0, n)
    assert empties > 1000
    got = pixels.combine(parts)
    assert np.all(total != 0)
    assert np.max(np.abs(got - total) / np.abs(total)) <= 1e-12


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
    px = pc.joined(pixels.resolving_power(centres, 1000.0), pixels.resolving_power(centres, 100.0))      # windows of 3-4 bins, and of the whole grid
    shifts = np.array([1.0, 1.0 - 150.0 / 299792.458, 1.0 + 150.0 / 299792.458, 0.9991])
    lens, margin = pc.window_lengths_and_margin(P, px, shifts)
    assert margin >= 1e-6 and lens.min() >= 2 and lens.max() == n
    tol = pc.tolerance(px, shifts)
    plain, pix, banded = Engine(P.static), Engine(P.static), Engine(P.static)
    pix.set_pixels(px)
    banded.set_bands(pixels.as_bands(px, shifts))
    for k in range(2):
        ref = plain.run(P.atm, P.opts)["spectrum"]
        out, spec = pix.run_pixels(P.atm, P.opts, shifts, spectrum=True)
        assert np.array_equal(spec, ref)
        pc.check_accuracy(P, px, shifts, out, spec, tol, what="opacity grid run %d vs reference" % k)
        pc.check_close(out, banded.run_bands(P.atm, P.opts).reshape(out.shape), tol, "opacity grid run %d vs run_bands" % k)
        assert np.array_equal(pix.run(P.atm, P.opts)["spectrum"], ref)
    plain.close(); pix.close(); banded.close()


def test_refusals_keep_the_previous_set(tmp_path):
    P = pc.make(tmp_path, "eclipse", nlines=10_000)
    E = Engine(P.static)
    lib = E._lib
    dp = _abi.c_double_p
    with pytest.raises(EngineError) as ei:             # no set installed
        E.run_pixels(P.atm, P.opts, [1.0])
    assert ei.value.code == -1
    good = pixels.Pixels([2510.0, 2520.0, 2530.0], [0.2, 0.3, 1.5], 4.0)
    E.set_pixels(good)
    before = E.run_pixels(P.atm, P.opts, pc.SHIFTS)
    assert np.all(before[..., 1] > 0)

    def with_pixel_2(centre=2530.0, fwhm=1.5, cut=4.0):
        return pixels.Pixels([2510.0, 2520.0, centre], [0.2, 0.3, fwhm], cut)

    bad = {
        "centre nan": with_pixel_2(centre=np.nan), "centre inf": with_pixel_2(centre=np.inf),
        "centre 0": with_pixel_2(centre=0.0), "centre < 0": with_pixel_2(centre=-2530.0),
        "fwhm nan": with_pixel_2(fwhm=np.nan), "fwhm inf": with_pixel_2(fwhm=np.inf),
        "fwhm 0": with_pixel_2(fwhm=0.0), "fwhm < 0": with_pixel_2(fwhm=-1.0),
    }
    for what, px in bad.items():
        with pytest.raises(EngineError) as ei:
            E.set_pixels(px)
        assert ei.value.code == -1 and "pixel 2" in str(ei.value), what
        assert np.array_equal(E.run_pixels(P.atm, P.opts, pc.SHIFTS), before), what
    for what, cut in (("cut 0", 0.0), ("cut < 0", -4.0), ("cut nan", np.nan), ("cut inf", np.inf)):
        with pytest.raises(EngineError) as ei:
            E.set_pixels(with_pixel_2(cut=cut))
        assert ei.value.code == -1 and "pixel" in str(ei.value) and "cut" in str(ei.value), what
    c = pixels.to_c(good)
    c.npix = -1
    assert lib.trx_set_pixels(E._h, C.byref(c)) == -1 and b"pixel" in lib.trx_last_error(E._h)
    c = pixels.to_c(good)
    c.fwhm = None
    assert lib.trx_set_pixels(E._h, C.byref(c)) == -1 and b"pixel" in lib.trx_last_error(E._h)
    c = pixels.to_c(good)
    c.centre = None
    assert lib.trx_set_pixels(E._h, C.byref(c)) == -1
    assert np.array_equal(E.run_pixels(P.atm, P.opts, pc.SHIFTS), before)
    # the run's own refusals
    out = np.zeros_like(before)
    sh = np.ascontiguousarray(pc.SHIFTS)

    def run(nshift, shift, dest):
        return lib.trx_run_pixels(E._h, C.byref(P.atm), C.byref(P.opts), None, nshift,
                                  shift.ctypes.data_as(dp) if shift is not None else None,
                                  dest.ctypes.data_as(dp) if dest is not None else None, None)

    assert run(0, sh, out) == -1 and run(-3, sh, out) == -1
    assert run(len(sh), None, out) == -1
    assert run(len(sh), sh, None) == -1
    for what, v in (("nan", np.nan), ("inf", np.inf), ("0", 0.0), ("< 0", -1.0)):
        s = sh.copy()
        s[4] = v
        assert run(len(s), s, out) == -1, what
        assert b"shift 4" in lib.trx_last_error(E._h), what
    assert np.all(out == 0)
    assert run(len(sh), sh, out) == 0
    assert np.array_equal(out, before)
    # run_bands and run_contrib know nothing of the pixels
    with pytest.raises(EngineError):
        E.run_bands(P.atm, P.opts)
    E.set_pixels(None)                                 # cleared: refused again
    with pytest.raises(EngineError):
        E.run_pixels(P.atm, P.opts, pc.SHIFTS)
    E.set_pixels(good)
    E.set_pixels(pixels.Pixels([], []))                # npix = 0 clears too
    with pytest.raises(EngineError):
        E.run_pixels(P.atm, P.opts, pc.SHIFTS)
    E.close()
    # a batch installs a set on every handle or on none
    B = Batch(P.static, ways=2)
    three = np.stack([pc.SHIFTS] * 3)
    with pytest.raises(EngineError):
        B.run_pixels([P.atm], P.opts, three[:1])
    B.set_pixels(good)
    ref = B.run_pixels([P.atm, P.atm, P.atm], P.opts, three)
    assert np.array_equal(ref[0], before) and np.array_equal(ref[2], before)
    with pytest.raises(EngineError) as ei:
        B.set_pixels(with_pixel_2(fwhm=0.0))
    assert "pixel 2" in str(ei.value)
    assert np.array_equal(B.run_pixels([P.atm, P.atm, P.atm], P.opts, three), ref)
    with pytest.raises(EngineError) as ei:             # a bad shift of one atmosphere fails the call and names it
        worse = three.copy()
        worse[1, 2] = 0.0
        B.run_pixels([P.atm, P.atm, P.atm], P.opts, worse)
    assert "shift 2" in str(ei.value)
    B.set_pixels(None)
    with pytest.raises(EngineError):
        B.run_pixels([P.atm], P.opts, three[:1])
    B.close()
