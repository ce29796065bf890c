"""The high-pass along the pixel axis without a device: tests/highpass_check.cpp, a stand-alone program over
transit_amd/csrc/trx_highpass.h (the arithmetic k_pixel_highpass runs per lane) and the high-pass functions of
transit_amd/csrc/trx_products.h, built with -ffp-contract=off under -fsanitize=address,undefined over exact-size heap
arrays -- and transit_amd.xcor's statement of the same definition, which the program's values must equal in every bit."""
import os
import subprocess

import numpy as np
import pytest

from bits import same_bits
from host_check import build_check

from transit_amd import xcor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 512                                             # kHpTile (the program asserts its own range; a wrong guess only tests less)


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("highpass_check", tmp_path_factory.mktemp("highpass_check"))


def test_refusals_layout_and_extents_under_sanitizers(check_exe):
    out = subprocess.run([check_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == ""                              # (no sanitizer report)
    lines = out.stdout.splitlines()
    assert not [line for line in lines if line.startswith("FAILED")]
    last = lines[-1].split()
    assert last[0] == "ok" and int(last[1]) > 60, lines[-20:]


def random_case(rng, lengths, nrow, gain):
    """pairs [nrow, npix, 2] of both signs with b > 0, b = 0 and b < 0 (a seventh of the pixels dead, and runs of them),
    an observed set over segments of the lengths given"""
    seg = xcor.segments(lengths)
    npix = int(seg[-1])
    pairs = np.stack([rng.uniform(-2.0, 3.0, (nrow, npix)), rng.uniform(0.1, 2.0, (nrow, npix))], axis=-1)
    dead = rng.random((nrow, npix)) < 1.0 / 7.0
    pairs[..., 1][dead] = rng.choice([0.0, -1.0, -0.0], size=int(dead.sum()))
    if npix > 40:
        pairs[0, 10:25, 1] = 0.0                           # a dead run wider than a small window
    ob = xcor.Observed(seg, np.zeros((1, npix)), None, rng.uniform(-1.5, 1.5, npix) if gain else None)
    return pairs, ob


def program_values(check_exe, tmp_path, pairs, ob, hp, name):
    src, dst = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
    with open(src, "wb") as f:
        np.array([pairs.shape[0], ob.npix, ob.nseg, hp.half, int(ob.gain is not None)], dtype=np.int64).tofile(f)
        ob.seg_first.tofile(f)
        hp.taps.tofile(f)
        if ob.gain is not None:
            ob.gain.tofile(f)
        np.ascontiguousarray(pairs).tofile(f)
    out = subprocess.run([check_exe, "values", src, dst], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-3000:] + out.stderr[-4000:]
    assert "0 differ from the literal definition" in out.stdout
    return np.fromfile(dst, dtype=np.float64).reshape(pairs.shape[0], ob.npix)


@pytest.mark.parametrize("half", [0, 1, 5, 70])
def test_values_are_the_numpy_definition_bit_for_bit(check_exe, tmp_path, half):
    """segments of 0, 1, 2, half, half + 1 and 2 half + 1 pixels (their ends inside every window) and one of two tiles and
    17; Gaussian-like, boxcar and random taps (zeros among them); with and without gains"""
    rng = np.random.default_rng(100 + half)
    lengths = [0, 1, 2, half, half + 1, 2 * half + 1, 0, 2 * TILE + 17, 3]
    tables = {"boxcar": np.ones(half + 1), "gauss": np.exp(-0.5 * (np.arange(half + 1) / max(half / 3.0, 1.0)) ** 2),
              "random": np.concatenate([[0.7], rng.uniform(0.0, 2.0, half) * (rng.random(half) > 0.2)])}
    for name, taps in tables.items():
        for gain in (False, True):
            pairs, ob = random_case(rng, lengths, 3, gain)
            hp = xcor.HighPass(taps)
            assert hp.half == half
            ref = xcor.highpass_reference(pairs, ob, hp)
            got = program_values(check_exe, tmp_path, pairs, ob, hp, "%s_%d_%d" % (name, half, gain))
            assert np.array_equal(np.isnan(ref), ~(pairs[..., 1] > 0))
            assert same_bits(got, ref), (name, gain, int(np.sum(got != ref)))
            if half == 0 and taps[0] == 1.0:             # (t g) / t is g for a power of two t; 0.7 g / 0.7 need not be
                live = ~np.isnan(got)
                assert np.all(got[live] == 0) and not np.any(np.signbit(got[live]))
    # a fully live set takes the full-window denominator away from the segments' ends: the same bits
    pairs, ob = random_case(rng, [2 * TILE + 17], 2, True)
    pairs[..., 1] = np.abs(pairs[..., 1]) + 0.5
    hp = xcor.HighPass(tables["gauss"])
    assert same_bits(program_values(check_exe, tmp_path, pairs, ob, hp, "live_%d" % half), xcor.highpass_reference(pairs, ob, hp))


def test_tap_tables():
    g = xcor.gaussian_highpass(80.0)
    assert g.half == 240 and g.taps[0] == 1.0 and np.all(np.diff(g.taps) < 0)
    assert np.array_equal(g.taps, np.exp(-(np.arange(241.0) ** 2) / (2.0 * 80.0 * 80.0)))
    assert xcor.gaussian_highpass(2.5, cut=2.0).half == 5 and xcor.gaussian_highpass(0.2).half == 0
    b = xcor.boxcar_highpass(7)
    assert b.half == 3 and np.array_equal(b.taps, np.ones(4))
    assert xcor.boxcar_highpass(1).half == 0
    for bad in (0, 4, -3):
        with pytest.raises(ValueError):
            xcor.boxcar_highpass(bad)
    with pytest.raises(ValueError):
        xcor.gaussian_highpass(0.0)
    c = b.to_c()
    assert c.half == 3 and c.taps[3] == 1.0


def test_half_zero_and_the_pairs_of_values():
    rng = np.random.default_rng(8)
    pairs, ob = random_case(rng, [5, 0, 50], 4, True)
    live = pairs[..., 1] > 0
    for hp in (xcor.HighPass([4.0]), xcor.boxcar_highpass(1), xcor.gaussian_highpass(0.3)):      # (t g) / t is g: t a power of two
        v = xcor.highpass_reference(pairs, ob, hp)
        assert hp.half == 0 and np.isnan(v[~live]).all() and np.all(v[live] == 0) and not np.any(np.signbit(v[live]))
    # a boxcar of 3 by hand, at a segment's end and beside a dead pixel
    ob1 = xcor.Observed([0, 4], np.zeros((1, 4)), None, np.array([2.0, 1.0, 1.0, 1.0]))
    p = np.array([[[1.0, 2.0], [3.0, 1.0], [5.0, 0.0], [7.0, 2.0]]])
    w = xcor.highpass_reference(p, ob1, xcor.boxcar_highpass(3))[0]
    assert w[0] == 1.0 - (1.0 + 3.0) / 2.0 and w[1] == 3.0 - (1.0 + 3.0) / 2.0 and np.isnan(w[2]) and w[3] == 0.0
    hp_pairs = xcor.highpass_pairs(w[None])
    assert hp_pairs.shape == (1, 4, 2) and np.array_equal(hp_pairs[0], [[-1.0, 1.0], [1.0, 1.0], [0.0, 0.0], [0.0, 1.0]])
    with pytest.raises(ValueError):
        xcor.highpass_reference(p[:, :3], ob1, xcor.boxcar_highpass(3))
