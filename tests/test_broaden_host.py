"""The rotational broadening without a device: transit_amd.broaden's reference and bound against cases worked by hand,
and the per-bin arithmetic the kernel runs (transit_amd/csrc/trx_broaden.h) on the CPU through tests/broaden_check.cpp,
block by block over exact-size tiles under -fsanitize=address,undefined."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import host_check

from transit_amd import broaden, pixels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = (1.037e-4, 1.3037e-3, 3.95e-6, 2e-6)          # the GPU tests': h 25-26, 325-333, 0-1, 0 on 2500 + 0.01 i, i < 6001


def test_rotation_is_v_over_c():
    b = broaden.Rotation(5.0, 0.3)
    assert b.beta == 5.0 / pixels.C_KMS and b.limb == 0.3
    assert broaden.Rotation.from_beta(1.037e-4).beta == 1.037e-4
    c = broaden.to_c(b)
    assert (c.kind, c.beta, c.limb) == (1, b.beta, 0.3)


def test_seven_bins_by_hand():
    """wn_i = 1000, wn_d = 1, beta = 0.0025: d_0 = 2.5, h = 2 everywhere.  limb = 0: w(x) = 2 sqrt(1 - x^2), so at bin 0
    x = 0.4, 0.8 give w = 2 sqrt(0.84), 1.2 and the window is one-sided; at bin 3, d = 2.5075."""
    S = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0])
    b = broaden.Rotation.from_beta(0.0025, 0.0)
    assert list(broaden.half_widths(1000.0, 1.0, 7, b.beta)) == [2] * 7
    B = broaden.reference(S, 1000.0, 1.0, b)
    w1 = 2.0 * math.sqrt(0.84)
    assert B[0] == pytest.approx((2.0 * 1.0 + w1 * 2.0 + 1.2 * 4.0) / (2.0 + w1 + 1.2), rel=1e-14)
    d = 1003 * 0.0025
    u1, u2 = 2.0 * math.sqrt(1.0 - (1.0 / d) ** 2), 2.0 * math.sqrt(1.0 - (2.0 / d) ** 2)
    assert B[3] == pytest.approx((2.0 * 8.0 + u1 * (4.0 + 16.0) + u2 * (2.0 + 32.0)) / (2.0 + 2.0 * u1 + 2.0 * u2), rel=1e-14)
    # bin 5 loses bin 7 only
    d = 1005 * 0.0025
    u1, u2 = 2.0 * math.sqrt(1.0 - (1.0 / d) ** 2), 2.0 * math.sqrt(1.0 - (2.0 / d) ** 2)
    assert B[5] == pytest.approx((2.0 * 32.0 + u1 * (16.0 + 64.0) + u2 * 8.0) / (2.0 + 2.0 * u1 + u2), rel=1e-14)
    # limb = 1: w(x) = (pi / 2) (1 - x^2); at bin 0, 0.84 and 0.36 times pi / 2, which cancels
    B1 = broaden.reference(S, 1000.0, 1.0, broaden.Rotation.from_beta(0.0025, 1.0))
    assert B1[0] == pytest.approx((1.0 + 0.84 * 2.0 + 0.36 * 4.0) / (1.0 + 0.84 + 0.36), rel=1e-14)
    assert np.array_equal(broaden.reference(S, 1000.0, 1.0, b, bins=[5, 0]), B[[5, 0]])


@pytest.mark.parametrize("limb", [0.0, 0.6, 1.0])
def test_constant_and_linear_spectra(limb):
    n, wn_i, wn_d = 400, 2505.0, 0.01
    b = broaden.Rotation.from_beta(1.037e-4, limb)
    h = broaden.half_widths(wn_i, wn_d, n, b.beta)
    assert h[0] == 25 and h[-1] == 26
    const = broaden.reference(np.full(n, 3.7), wn_i, wn_d, b)
    # (to rounding: numerator and denominator are rounded once each, then the quotient)
    assert np.max(np.abs(const - 3.7)) <= 2 * 3.7 * 2.0 ** -52
    lin = 5.0 + 0.25 * np.arange(n)
    B = broaden.reference(lin, wn_i, wn_d, b)
    i = np.arange(n)
    inside = (i - h >= 0) & (i + h < n)
    assert inside.sum() == n - 25 - 26
    assert np.max(np.abs(B[inside] - lin[inside]) / lin[inside]) <= 2 * 2.0 ** -52      # symmetric window: unchanged
    assert np.all(B[:25] > lin[:25]) and np.all(B[-26:] < lin[-26:])                # one-sided at the ends


@pytest.mark.parametrize("limb", [0.0, 0.6, 1.0])
def test_spike_comes_back_as_the_normalised_kernel(limb):
    n, wn_i, wn_d, j = 200, 2500.0, 0.01, 90
    b = broaden.Rotation.from_beta(1.037e-4, limb)
    h, d = broaden._halves(wn_i, wn_d, n, b.beta)
    c1, c2 = broaden.weights(limb)
    S = np.zeros(n)
    S[j] = 2.0
    B = broaden.reference(S, wn_i, wn_d, b)
    for i in range(n):
        k = abs(i - j)
        if k > h[i]:
            assert B[i] == 0.0
            continue
        w = lambda q: c1 * math.sqrt(max(0.0, 1.0 - (q * wn_d / d[i]) ** 2)) + c2 * max(0.0, 1.0 - (q * wn_d / d[i]) ** 2)
        den = w(0) + sum(w(q) * ((i - q >= 0) + (i + q < n)) for q in range(1, h[i] + 1))
        assert B[i] == pytest.approx(2.0 * w(k) / den, rel=1e-13), i
    # the two pure profiles: a spike k bins from bin i against a spike on it is w(x_k) / w(0)
    i = 100
    centre = np.zeros(n); centre[i] = 1.0
    b0 = broaden.reference(centre, wn_i, wn_d, b, bins=[i])[0]
    for k in (1, 7, 20, 25):
        off = np.zeros(n); off[i + k] = 1.0
        x2 = (k * wn_d / d[i]) ** 2
        ratio = broaden.reference(off, wn_i, wn_d, b, bins=[i])[0] / b0
        if limb == 0.0:
            assert ratio == pytest.approx(math.sqrt(1.0 - x2), rel=1e-13)
        elif limb == 1.0:
            assert ratio == pytest.approx(1.0 - x2, rel=1e-13)
        else:
            assert 1.0 - x2 < ratio < math.sqrt(1.0 - x2)


def test_no_half_width_is_the_identity():
    rng = np.random.default_rng(3)
    S = np.exp(rng.normal(size=6001))
    b = broaden.Rotation.from_beta(2e-6, 0.6)
    assert not broaden.half_widths(2500.0, 0.01, 6001, b.beta).any()
    assert np.array_equal(broaden.reference(S, 2500.0, 0.01, b), S)


def test_half_widths_do_not_decrease():
    for beta, lo, hi in zip(BETAS, (25, 325, 0, 0), (26, 333, 1, 0)):
        h = broaden.half_widths(2500.0, 0.01, 6001, beta)
        assert h[0] == lo and h[-1] == hi and np.all(np.diff(h) >= 0), beta
    rng = np.random.default_rng(11)
    for _ in range(50):
        wn_i, wn_d, beta = rng.uniform(100, 30000), 10 ** rng.uniform(-3, 0), 10 ** rng.uniform(-6, -3.5)
        h = broaden.half_widths(wn_i, wn_d, 5000, beta)
        assert np.all(np.diff(h) >= 0) and h[0] >= 0


def test_a_double_walk_in_the_kernels_order_is_inside_the_bound():
    """bound() is derived, not tuned: a plain double evaluation, centre first and pairs ascending, must sit well inside."""
    n, wn_i, wn_d = 700, 2500.0, 0.01
    rng = np.random.default_rng(7)
    S = np.exp(rng.normal(size=n))
    for beta, limb in ((1.037e-4, 0.6), (1.3037e-3, 0.0), (3.95e-6 * 1.1, 1.0)):
        b = broaden.Rotation.from_beta(beta, limb)
        h, d = broaden._halves(wn_i, wn_d, n, beta)
        c1, c2 = broaden.weights(limb)
        ref = broaden.reference(S, wn_i, wn_d, b)
        tol = broaden.bound(S, wn_i, wn_d, b, ref=ref)
        got = S.copy()
        for i in (int(q) for q in np.flatnonzero(h > 0)):
            num, den = (c1 + c2) * S[i], c1 + c2
            for k in range(1, h[i] + 1):
                x = (k * wn_d) / d[i]
                t = max(0.0, 1.0 - x * x)
                w = c1 * math.sqrt(t) + c2 * t
                s = (S[i - k] if i - k >= 0 else 0.0) + (S[i + k] if i + k < n else 0.0)
                num += w * s
                den += w * ((i - k >= 0) + (i + k < n))
            got[i] = num / den
        ratio = np.abs(got - ref) / tol
        print("beta %g limb %g: largest err/tol %.3f" % (beta, limb, ratio.max()))
        # (wide windows sit far inside; at h = 1 the one weight is on the profile's edge, where E_i is most of the bound)
        assert ratio.max() < (0.1 if h.max() > 1 else 0.7) and np.all(tol < 1e-11 * np.abs(ref))


def build_check(tmp, short):
    return host_check.build_check("broaden_check", tmp, public_headers=False, defines=["BROADEN_TILE_SHORT=%d" % short], exe_name="broaden_check_%d" % short)


def test_kernel_arithmetic_on_exact_tiles_under_sanitizers(tmp_path):
    """Every block of the GPU tests' four betas (three limb coefficients each) over a heap tile of exactly the bins the
    kernel stages: no read outside it, every bin inside its bound against long double, and the halo of the grid's first
    and last block as half_widths gives it."""
    out = subprocess.run([build_check(tmp_path, 0)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "72012 bins, 0 outside their bound, 0 decreasing half-widths" in out.stdout
    for beta in BETAS:
        h = broaden.half_widths(2500.0, 0.01, 6001, beta)
        first = re.search(r"beta %g: block 0 bins \[0, 255\] H (\d+) stages \[(\d+), (\d+)\]" % beta, out.stdout)
        last = re.search(r"beta %g: block 23 bins \[5888, 6000\] H (\d+) stages \[(\d+), (\d+)\]" % beta, out.stdout)
        assert first and last, out.stdout
        assert [int(x) for x in first.groups()] == [h[255], 0, 255 + h[255]]
        assert [int(x) for x in last.groups()] == [h[6000], 5888 - h[6000], 6000]
        m = re.search(r"beta %g: h (\d+)\.\.(\d+), 24 blocks, (\d+) copied bins, largest err/tol ([\d.]+)" % beta, out.stdout)
        assert m and (int(m.group(1)), int(m.group(2))) == (h[0], h[-1]) and int(m.group(3)) == 3 * int((h == 0).sum())
        assert float(m.group(4)) < 1.0


def test_a_tile_one_bin_short_is_an_out_of_bounds_read_on_the_cpu(tmp_path):
    out = subprocess.run([build_check(tmp_path, 1)], capture_output=True, text=True)
    assert out.returncode != 0 and "heap-buffer-overflow" in out.stderr, out.stdout + out.stderr
