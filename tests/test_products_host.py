"""The host side of the run products without a device: the refusal table, the band and filter layouts and the buffer
extents of transit_amd/csrc/trx_products.h through tests/products_check.cpp, a stand-alone program over exact-size heap
arrays under -fsanitize=address,undefined -- and the GAUSS range rule it holds against bands.gauss_range, its Python mirror."""
import os
import subprocess

import numpy as np
import pytest

from host_check import build_check

from transit_amd import bands

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("products_check", tmp_path_factory.mktemp("products_check"))


@pytest.fixture(scope="module")
def whole_run(check_exe):
    """the program's own checks, run once: its output lines"""
    out = subprocess.run([check_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == ""                              # (no sanitizer report)
    return out.stdout.splitlines()


def gauss_lines(lines):
    """[((wn_i, wn_d, nwn, centre, fwhm, cut), (first, last))] of the program's "gauss" lines"""
    got = []
    for line in lines:
        w = line.split()
        if w and w[0] == "gauss":
            f = float.fromhex
            got.append(((f(w[1]), f(w[2]), int(w[3]), f(w[4]), f(w[5]), f(w[6])), (int(w[7]), int(w[8]))))
    return got


def test_refusals_layouts_and_extents_under_sanitizers(whole_run):
    last = whole_run[-1].split()
    assert last[0] == "ok" and int(last[1]) > 300, whole_run[-20:]
    assert not [line for line in whole_run if line.startswith("FAILED")]


def test_layout_gauss_bands_are_the_mirrors_ranges(whole_run):
    """the GAUSS bands of the layout cases: clipped at 0 and at nwn, off either end, centres of +-1e300"""
    got = gauss_lines(whole_run)
    assert len(got) >= 12
    assert any(a[3] == 1e300 for a, _ in got) and any(a[3] == -1e300 for a, _ in got)
    for args, rng in got:
        assert bands.gauss_range(*args) == rng, args
    ranges = [r for _, r in got]
    assert (0, 0) in ranges and (5000, 5000) in ranges and (0, 5000) in ranges
    assert any(a == 0 and 0 < z < 5000 for a, z in ranges) and any(0 < a < 5000 and z == 5000 for a, z in ranges)


def test_gauss_range_mirror_on_the_host_tests_cases(check_exe, tmp_path):
    """bands.gauss_range against the C++ rule on the numbers of tests/test_bands_host.py::test_gauss_range_rule"""
    n, wn_i, wn_d = 400, 2500.0, 0.5
    wn = wn_i + np.arange(n) * wn_d
    rng = np.random.default_rng(3)
    cases = [(float(c), float(f), float(k)) for c, f, k in zip(rng.uniform(2490, 2710, 200), rng.uniform(0.01, 5, 200), rng.uniform(0.5, 6, 200))]
    for fwhm, cut in ((0.5 * bands.FWHM_PER_SIGMA, 4.0), (0.25 * bands.FWHM_PER_SIGMA, 2.0)):
        cases += [(float(wn[k]), fwhm, cut) for k in (0, 1, 3, 200, n - 4, n - 2, n - 1)]
    cases += [(wn[0] - 1000.0, 1.0, 4.0), (wn[-1] + 1000.0, 1.0, 4.0), (wn[0] - 10.0, 100.0, 4.0), (1e300, 1.0, 4.0), (-1e300, 1.0, 4.0)]
    path = tmp_path / "gauss.txt"
    with open(path, "w") as f:
        for c, w, k in cases:
            f.write("%s %s %d %s %s %s\n" % (wn_i.hex(), wn_d.hex(), n, float(c).hex(), float(w).hex(), float(k).hex()))
    out = subprocess.run([check_exe, "gauss", str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-4000:]
    got = gauss_lines(out.stdout.splitlines())
    assert len(got) == len(cases)
    for (c, w, k), (args, r) in zip(cases, got):
        assert args == (wn_i, wn_d, n, c, w, k)
        assert bands.gauss_range(wn_i, wn_d, n, c, w, k) == r, (c, w, k)
    assert got[200 + 3][1] == (196, 205) and got[200 + 1][1] == (0, 6)      # the exact edges are in (sigma = 0.5: 4 bins either side)
