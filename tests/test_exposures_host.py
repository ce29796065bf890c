"""The exposure table without a device: the refusals, extents and range rule of transit_amd/csrc/trx_exposures.h through
tests/exposures_check.cpp, a stand-alone program over exact-size heap arrays under -fsanitize=address,undefined; the range
rule held against exposures.exposed_range, its Python mirror; the definition (exposures.reference) held against what it
stands for, the average of plain pixel values over the Doppler factors of the exposure (exposures.subshift_average); and
the ABI: the struct's size and the four exported symbols."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from host_check import build_check

from transit_amd import _abi, bands, build, exposures, pixels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("exposures_check", tmp_path_factory.mktemp("exposures_check"))


@pytest.fixture(scope="module")
def whole_run(check_exe):
    """the program's own checks, run once: its output lines"""
    out = subprocess.run([check_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == ""                              # (no sanitizer report)
    return out.stdout.splitlines()


def range_lines(lines):
    """[((wn_i, wn_d, nwn, cut, centre_obs, fwhm_obs, shift, eta), (centre, sigma, d), (first, last))] of the "range" lines"""
    got = []
    for line in lines:
        w = line.split()
        if w and w[0] == "range":
            f = float.fromhex
            got.append(((f(w[1]), f(w[2]), int(w[3]), f(w[4]), f(w[5]), f(w[6]), f(w[7]), f(w[8])), (f(w[9]), f(w[10]), f(w[11])),
                        (int(w[12]), int(w[13]))))
    return got


def mirror(args):
    wn_i, wn_d, nwn, cut, c, f, s, eta = args
    return exposures.exposed_range(wn_i, wn_d, nwn, c / s, f / s, cut, eta)


def test_refusals_extents_and_ranges_under_sanitizers(whole_run):
    last = whole_run[-1].split()
    assert last[0] == "ok" and int(last[1]) > 60, whole_run[-20:]
    assert not [line for line in whole_run if line.startswith("FAILED")]


def test_the_programs_edge_ranges_are_the_mirrors(whole_run):
    """clipped at 0 and at nwn, off either end, centres of +-1e300, eta = 0 and eta = TRX_SMEAR_MAX, a centre that overflows"""
    got = range_lines(whole_run)
    assert len(got) >= 70
    etas = {a[7] for a, _, _ in got}
    assert 0.0 in etas and exposures.SMEAR_MAX in etas and _abi.SMEAR_MAX == exposures.SMEAR_MAX
    assert any(a[4] == 1e300 for a, _, _ in got) and any(a[4] == -1e300 for a, _, _ in got)
    for args, (centre, sigma, d), rng in got:
        assert mirror(args) == rng, args
        if args[7] == 0.0:                               # the plain Gaussian's bins
            assert d == 0.0 and rng == bands.gauss_range(args[0], args[1], args[2], args[4] / args[6], args[5] / args[6], args[3]), args
        elif math.isfinite(centre):
            assert d == centre * args[7]
    ranges = [r for _, _, r in got]
    assert (0, 0) in ranges and (5000, 5000) in ranges and (0, 5000) in ranges
    assert any(a == 0 and 0 < z < 5000 for a, z in ranges) and any(0 < a < 5000 and z == 5000 for a, z in ranges)


def test_range_mirror_on_random_cases(check_exe, tmp_path):
    """exposures.exposed_range against the C++ rule on 300 random (centre, fwhm, cut, eta) and the edges of
    tests/test_products_host.py's Gaussian cases, each at eta = 0, a small eta and TRX_SMEAR_MAX"""
    n, wn_i, wn_d = 400, 2500.0, 0.5
    wn = wn_i + np.arange(n) * wn_d
    rng = np.random.default_rng(11)
    cases = [(float(c), float(f), float(k), float(s), float(e)) for c, f, k, s, e in
             zip(rng.uniform(2490, 2710, 300), rng.uniform(0.01, 5, 300), rng.uniform(0.5, 6, 300), rng.uniform(0.9995, 1.0005, 300),
                 10.0 ** rng.uniform(-9, -2, 300))]
    edges = []
    for fwhm, cut in ((0.5 * bands.FWHM_PER_SIGMA, 4.0), (0.25 * bands.FWHM_PER_SIGMA, 2.0)):
        edges += [(float(wn[k]), fwhm, cut) for k in (0, 1, 3, 200, n - 4, n - 2, n - 1)]
    edges += [(wn[0] - 1000.0, 1.0, 4.0), (wn[-1] + 1000.0, 1.0, 4.0), (wn[0] - 10.0, 100.0, 4.0), (1e300, 1.0, 4.0), (-1e300, 1.0, 4.0)]
    for eta in (0.0, 3e-6, exposures.SMEAR_MAX):
        cases += [(c, f, k, 1.0, eta) for c, f, k in edges]
    path = tmp_path / "range.txt"
    with open(path, "w") as f:
        for c, w, k, s, e in cases:
            f.write("%s %s %d %s %s %s %s %s\n" % (wn_i.hex(), wn_d.hex(), n, k.hex(), float(c).hex(), float(w).hex(), s.hex(), float(e).hex()))
    out = subprocess.run([check_exe, "range", str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-4000:]
    got = range_lines(out.stdout.splitlines())
    assert len(got) == len(cases)
    lengths = set()
    for (c, w, k, s, e), (args, _, r) in zip(cases, got):
        assert args == (wn_i, wn_d, n, k, c, w, s, e)
        assert mirror(args) == r, args
        lengths.add(r[1] - r[0])
    assert len(lengths) > 30 and 0 in lengths and max(lengths) > 300
    # the exact edges are in at eta = 0 (sigma = 0.5: 4 bins either side), and the smear moves them out
    assert got[300 + 3][1:] == ((wn[200], 0.5, 0.0), (196, 205)) and got[300 + 1][2] == (0, 6)
    assert got[300 + len(edges) + 3][2] == (196, 205)                  # d = 7.8e-3 cm-1: below one bin, the same bins
    assert got[300 + 2 * len(edges) + 3][2] == (144, 257)              # d = 26 cm-1 = 52 bins


def synthetic_spectrum(wn, seed=7):
    """A positive spectrum with absorption lines of Gaussian width 0.01 .. 0.05 cm-1, 2 to 12 per cent deep, on a sloping
    continuum.  The depth matters to the comparison below: a pixel value cut at 4 sigma leaves erfc(4 / sqrt 2) = 6.3e-5 of
    the Gaussian out, the definition's wider window leaves out less, and the two means differ by at most that mass times
    the spectrum's relative range over the window -- with a range below 0.3 (a few blended lines of this depth) under 2e-5."""
    rng = np.random.default_rng(seed)
    s = 1.0 + 1e-3 * (wn - wn[0])
    for nu0, depth, width in zip(rng.uniform(wn[0], wn[-1], 150), rng.uniform(0.02, 0.12, 150), rng.uniform(0.01, 0.05, 150)):
        s = s * (1.0 - depth * np.exp(-0.5 * ((wn - nu0) / width) ** 2))
    return s


@pytest.mark.parametrize("R", [3000.0, 20000.0, 100000.0])
def test_definition_against_the_subshift_average(R):
    """The definition against the physics: on 6001 bins the box-convolved Gaussian over the window cut at 4 sigma + d,
    with the first-order d, against the mean of plain pixel values over 401 sub-shifts, for full velocity changes of 0.5,
    2 and 8 km/s.  Relative difference <= 2e-5: on the definition alone the worst case is 5.6e-6 (window truncation and the
    first-order d), and the limit is 3.5 times that."""
    wn_i, wn_d, n = 2500.0, 0.01, 6001
    wn = wn_i + np.arange(n) * wn_d
    spec = synthetic_spectrum(wn)
    assert spec.min() > 0 and (spec.max() - spec.min()) / spec.mean() < 0.3
    px = pixels.resolving_power(np.linspace(2505, 2555, 40) + 0.37 * wn_d, R, 4.0)
    dv = np.array([0.5, 2.0, 8.0])
    shifts = np.array([1.0 - 37.5 / pixels.C_KMS, 1.0, 1.0 + 150.0 / pixels.C_KMS])
    ex = exposures.Exposures(smear=dv / (2.0 * pixels.C_KMS))
    ref = exposures.reference(spec, wn_i, wn_d, n, px, shifts, ex)
    assert np.all(ref[..., 1] > 0)
    val = ref[..., 0] / ref[..., 1]
    avg = exposures.subshift_average(spec, wn_i, wn_d, n, px, shifts, ex, nsub=401)
    worst = float(np.max(np.abs(val - avg) / np.abs(avg)))
    print("R = %g: worst relative difference %.3e" % (R, worst))
    assert worst <= 2e-5
    # and the smear is not a no-op at this resolution: the plain pixel differs by more where it matters
    if R == 100000.0:
        plain = pixels.value(pixels.reference(spec, wn_i, wn_d, n, px, shifts))
        assert np.max(np.abs(plain[2] - avg[2]) / np.abs(avg[2])) > 1e-3


def test_reference_rows_without_smear_and_the_scale():
    wn_i, wn_d, n = 2500.0, 0.01, 6001
    wn = wn_i + np.arange(n) * wn_d
    spec = synthetic_spectrum(wn, 3)
    px = pixels.resolving_power(np.linspace(2499.9, 2560.1, 9), 20000.0, 4.0)      # (the outer two hang over the grid's ends)
    shifts = np.array([1.0, 1.00001, 0.99999])
    plain = pixels.reference(spec, wn_i, wn_d, n, px, shifts)
    ex = exposures.Exposures(scale=[1.0, -0.25, 0.0], smear=[0.0, 0.0, 1e-6])
    ref = exposures.reference(spec, wn_i, wn_d, n, px, shifts, ex)
    assert np.array_equal(ref[0], plain[0])
    assert np.array_equal(ref[1, :, 1], plain[1, :, 1]) and np.array_equal(ref[1, :, 0], -0.25 * plain[1, :, 0])
    assert np.all(ref[2, :, 0] == 0) and np.all(ref[2, :, 1] > 0)
    # a shard: the partial pairs add up, and a pair with no bin there is (+0, +0) whatever the scale
    parts = [exposures.reference(spec[a:z], wn_i, wn_d, n, px, shifts, ex, lo=a) for a, z in ((0, 1500), (1500, 3777), (3777, n))]
    total = parts[0] + parts[1] + parts[2]
    assert np.max(np.abs(total - ref) / np.maximum(np.abs(ref), 1e-300)) < 1e-13
    empty = parts[0][:, -1]
    assert np.all(empty == 0) and not np.any(np.signbit(empty))
    assert exposures.smear_half(200.0, 0.0, 0.01) == pytest.approx(200.0 * 2 * math.pi * 0.01 / (2 * pixels.C_KMS))
    assert exposures.smear_half(200.0, 0.25, 0.01) < 1e-18 and exposures.smear_half(-200.0, 0.5, 0.01) > 0


def test_abi_struct_and_symbols():
    assert ctypes.sizeof(_abi.TrxExposures) == 24
    path = build.lib_path("libtransit_hip.so")
    if not os.path.exists(path):
        build.build_hip()
    lib = ctypes.CDLL(path)
    for name in ("trx_set_exposures", "trx_run_exposed", "trx_batch_set_exposures", "trx_run_batch_exposed"):
        assert hasattr(lib, name), name
    lib.trx_abi_version.restype = ctypes.c_int
    assert lib.trx_abi_version() == 5
    assert b"k_pixel_pairs_exposed" in open(path, "rb").read()
    # refused without a handle, before anything is touched
    _abi.bind(lib, _abi.HIP_HEADER, "trx_")
    assert lib.trx_set_exposures(None, None) == -1
