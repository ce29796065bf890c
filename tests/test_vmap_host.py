"""The detection map without a device: transit_amd.xcor's definitions (trail_statistic, map_from_per, map_reference,
map_bound) against cases worked by hand and against the older xcor.velocity_map, and the arithmetic the two kernels run
(transit_amd/csrc/trx_vmap.h) on the CPU through tests/vmap_check.cpp, a stand-alone program over exact-size buffers
under -fsanitize=address,undefined."""
import math
import os
import subprocess

import numpy as np
import pytest

from host_check import build_check

from transit_amd import xcor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
STATS = ("ccf", "loglike_bl19", "chi2")


def row(f, g, w=None):
    """the seven moments of the pixels (f, g, w) of one segment"""
    f, g = np.asarray(f, dtype=float), np.asarray(g, dtype=float)
    w = np.ones_like(f) if w is None else np.asarray(w, dtype=float)
    return np.array([f.size, w.sum(), (w * g).sum(), (w * g * g).sum(), (w * f).sum(), (w * f * g).sum(), (w * f * f).sum()])


ORDINARY = row([1, 2, 4], [1, 3, 2])          # <f> = 7/3, <g> = 2, sf2 = 14/9, sg2 = 2/3, R = 1/3
OTHER = row([2, 0, 1, 5], [1, 1, 3, 4])       # <f> = 2, <g> = 9/4, sf2 = 7/2, sg2 = 27/16, R = 25/4 - 9/2 = 7/4
ONE_PIXEL = row([3], [2])                     # n = 1
FLAT_MODEL = row([1, 2, 4], [2, 2, 2])        # sg2 = 0
EMPTY = np.zeros(7)
CCF_ORDINARY = (1 / 3) / math.sqrt((14 / 9) * (2 / 3))
CCF_OTHER = (7 / 4) / math.sqrt((7 / 2) * (27 / 16))


def hand_trail():
    """[2 lags][2 exposures][3 segments]: (0, 0) one ordinary row among two skipped, (0, 1) all skipped, (1, 0) two
    ordinary rows around a skipped one, (1, 1) the empty row first"""
    return np.array([[[ORDINARY, ONE_PIXEL, FLAT_MODEL], [ONE_PIXEL, FLAT_MODEL, EMPTY]],
                     [[OTHER, FLAT_MODEL, ORDINARY], [EMPTY, OTHER, ONE_PIXEL]]])


def test_rows_by_hand_and_skipped_rows():
    trail = hand_trail()
    vm = xcor.VelocityMap([-1.0, 1.0], [0.5], [0.0], [1.0, -1.0])
    per = xcor.trail_statistic(trail, vm)
    assert per.shape == (2, 2)
    assert per[0, 0] == pytest.approx(CCF_ORDINARY, rel=1e-15)
    assert per[0, 1] == 0.0 and not np.signbit(per[0, 1])              # every row skipped: +0
    assert per[1, 0] == pytest.approx(CCF_OTHER + CCF_ORDINARY, rel=1e-15)
    assert per[1, 1] == pytest.approx(CCF_OTHER, rel=1e-15)
    # x = 0.5 at exposure 0 (t = 0.75), -0.5 at exposure 1 (t = 0.25)
    m = xcor.map_from_per(per, vm)
    want = (per[0, 0] + 0.75 * (per[1, 0] - per[0, 0])) + (per[0, 1] + 0.25 * (per[1, 1] - per[0, 1]))
    assert m.shape == (1, 1) and m[0, 0] == want
    assert np.array_equal(xcor.map_reference(trail, vm), m)
    # the other two statistics of the ordinary row: sum (f - 2 g + 1)^2 = 0 + 9 + 1; arg = 14/9 - 1/3 + 1/6 = 25/18
    chi = xcor.VelocityMap([-1.0, 1.0], [0.5], [0.0], [1.0, -1.0], stat="chi2", a=2.0, b=-1.0)
    assert xcor.trail_statistic(trail[:1, :1, :1], xcor.VelocityMap([0.0], [0.0], [0.0], [0.0], stat="chi2", a=2.0, b=-1.0))[0, 0] == 10.0
    # (chi-square is defined for every row: the empty one adds its zero, the one-pixel row (3 - 4 + 1)^2 = 0)
    assert xcor.trail_statistic(trail, chi)[0, 1] == pytest.approx(0.0 + (1 - 3) ** 2 + (2 - 3) ** 2 + (4 - 3) ** 2 + 0.0, abs=1e-13)
    bl = xcor.VelocityMap([-1.0, 1.0], [0.5], [0.0], [1.0, -1.0], stat="loglike_bl19", scale=0.5)
    got = xcor.trail_statistic(trail, bl)
    assert got[0, 0] == pytest.approx(-1.5 * math.log(25 / 18), rel=1e-14)
    assert got[0, 1] == 0.0 and not np.signbit(got[0, 1])
    # a non-positive argument of the logarithm is skipped too: f = g gives sf2 = sg2 = R, arg = 0 at scale 1
    same = np.array([[[row([1, 2, 4], [1, 2, 4]), ORDINARY]]])
    one = xcor.VelocityMap([0.0], [0.0], [0.0], [0.0], stat="loglike_bl19", scale=1.0)
    assert xcor.trail_statistic(same, one)[0, 0] == xcor.loglike_bl19(ORDINARY, 1.0)


def test_nodes_the_last_node_and_one_ulp_outside():
    per = np.array([[1.0], [3.0], [7.0]])
    vsys = [2.0, 4.0, np.nextafter(4.0, np.inf), 1.0, 0.0, np.nextafter(0.0, -np.inf), np.nextafter(4.0, 0.0)]
    vm = xcor.VelocityMap([0.0, 2.0, 4.0], [10.0, -3.0], vsys, [0.0])       # orbit = 0: x = vsys for every Kp
    m = xcor.map_from_per(per, vm)
    t = (np.nextafter(4.0, 0.0) - 2.0) / 2.0
    want = [3.0, 7.0, np.nan, 2.0, 1.0, np.nan, 3.0 + t * 4.0]
    assert m.shape == (2, 7)
    assert np.array_equal(m, np.array([want, want]), equal_nan=True)
    # an offset moves every exposure's velocity; a velocity that is not finite is outside
    off = xcor.VelocityMap([0.0, 2.0, 4.0], [0.0], [1.0, 3.5], [0.0], offset=[0.5])
    assert np.array_equal(xcor.map_from_per(per, off), [[1.0 + 0.75 * 2.0, 7.0]])
    inf = xcor.VelocityMap([0.0, 2.0, 4.0], [0.0], [1.0], [0.0], offset=[np.inf])
    assert np.isnan(xcor.map_from_per(per, inf)[0, 0])
    assert np.all(np.isnan(xcor.map_bound(np.ones((3, 1, 1, 7)), inf)))


def test_one_lag():
    vm = xcor.VelocityMap([5.0], [1.0], [5.0, 5.5], [0.0, 0.0])
    assert np.array_equal(xcor.map_from_per(np.array([[2.0, 3.0]]), vm), [[5.0, np.nan]], equal_nan=True)
    trail = np.stack([ORDINARY, OTHER]).reshape(1, 2, 1, 7)
    assert xcor.map_reference(trail, vm)[0, 0] == xcor.ccf(ORDINARY) + xcor.ccf(OTHER)
    b = xcor.map_bound(trail, vm)
    assert b[0, 0] > 0 and np.isnan(b[0, 1])


def test_to_c_mirrors_the_map():
    vm = xcor.VelocityMap([-3.0, 0.0, 3.0], [1.0, 2.0], [0.0], [0.1, 0.2, 0.3, 0.4], offset=[0.0] * 4, stat="chi2", a=1.5, b=0.25)
    c = vm.to_c()
    assert (c.stat, c.nlag, c.nkp, c.nvsys, c.p0, c.p1) == (3, 3, 2, 1, 1.5, 0.25)
    assert [c.lag[k] for k in range(3)] == [xcor._pixels.shift(v) for v in (-3.0, 0.0, 3.0)] and c.lag[1] == 1.0
    assert c.orbit[3] == 0.4 and c.offset[0] == 0.0 and c.lag_kms[2] == 3.0
    assert not xcor.VelocityMap([0.0], [1.0], [0.0], [0.0]).to_c().offset               # (a NULL pointer)
    assert xcor.VelocityMap([0.0], [1.0], [0.0], [0.0], stat="loglike_bl19", scale=0.7).params == (0.7, 0.0)
    with pytest.raises(ValueError):
        xcor.VelocityMap([0.0], [1.0], [0.0], [0.0], stat="median")
    with pytest.raises(ValueError):
        xcor.VelocityMap([0.0], [1.0], [0.0], [0.0, 1.0], offset=[0.0])


def random_trail(rng, nlag, nexp, nseg):
    """moments of random data, one row in nine with fewer than two pixels"""
    shape = (nlag, nexp, nseg)
    n = rng.integers(0, 50, shape).astype(float)
    n[rng.random(shape) < 0.1] = 1.0
    g, f = rng.normal(size=shape), rng.normal(size=shape)
    m = np.zeros(shape + (7,))
    m[..., 0] = n
    m[..., 1] = n * rng.uniform(0.5, 2.0, shape)
    m[..., 2], m[..., 4] = m[..., 1] * g, m[..., 1] * f
    m[..., 3] = m[..., 1] * (g * g + rng.uniform(0.1, 1.0, shape))
    m[..., 6] = m[..., 1] * (f * f + rng.uniform(0.1, 1.0, shape))
    m[..., 5] = m[..., 1] * (f * g + rng.uniform(-0.1, 0.1, shape))
    m[n == 1.0, 3] = m[n == 1.0, 2] ** 2 / m[n == 1.0, 1]                # (one pixel: no variance)
    return m


def the_map(stat, nexp=7, offset=False):
    """the GPU tests' grid: 55 lags, seven Kp by five Vsys, the Kp = 250 row outside and Kp = 190 outside at Vsys = +-12"""
    kms, _ = xcor.lag_grid(-81.0, 81.0, 3.0)
    phase = np.linspace(-0.06, 0.06, nexp)
    off = 0.3 * np.cos(np.arange(nexp)) if offset else None
    return xcor.VelocityMap(kms, [40.0, 70.0, 100.0, 130.0, 160.0, 190.0, 250.0], np.arange(-12.0, 13.0, 6.0), np.sin(2 * np.pi * phase),
                            offset=off, stat=stat, scale=0.9, a=1.1, b=0.2)


@pytest.mark.parametrize("stat", STATS)
def test_map_reference_against_velocity_map(stat):
    rng = np.random.default_rng(5)
    vm = the_map(stat)
    vp = vm.vsys[None, :, None] + vm.kp[:, None, None] * vm.orbit[None, None, :]
    outside = np.zeros((7, 5), dtype=bool)
    outside[6], outside[5, [0, 4]] = True, True
    # two segments: nansum adds them in order too
    trail = random_trail(rng, 55, 7, 2)
    ref, old = xcor.map_reference(trail, vm), xcor.velocity_map(trail, vm.lag_kms, vp, stat=vm.statistic)
    assert np.array_equal(np.isnan(ref), outside)
    assert np.array_equal(ref, old, equal_nan=True)
    # forty: pairwise against in order
    trail = random_trail(rng, 55, 7, 40)
    ref, old = xcor.map_reference(trail, vm), xcor.velocity_map(trail, vm.lag_kms, vp, stat=vm.statistic)
    bound = xcor.map_bound(trail, vm)
    assert np.array_equal(np.isnan(ref), outside) and np.array_equal(np.isnan(old), outside) and np.array_equal(np.isnan(bound), outside)
    ratio = float(np.nanmax(np.abs(ref - old) / bound))
    print("%s, 40 segments: worst |map_reference - velocity_map| / map_bound %.4f" % (stat, ratio))
    assert ratio <= 1.0 and np.any(ref != old)
    # the bound is below what the interface promises at the most
    a = np.nansum(np.abs(vm.statistic(trail)), axis=2)
    _, k, _ = xcor._locate(vm.lag_kms, xcor._tracks(vm))
    s = sum(a[k[..., v], v] + a[k[..., v] + 1, v] for v in range(7))
    assert np.all(bound[~outside] <= ((40 + 7 + 16) * EPS * s)[~outside])
    assert np.all(xcor.per_bound(trail, vm) <= (40 + 5) * EPS * a)


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("vmap_check", tmp_path_factory.mktemp("vmap_check"), public_headers=False)


def run_check(exe, path, trail, vm):
    """(per, map) of tests/vmap_check.cpp for a trail and a map"""
    hexes = lambda x: " ".join(float(v).hex() for v in np.asarray(x, dtype=np.float64).ravel())
    p0, p1 = vm.params
    with open(path, "w") as f:
        f.write("%d %s %s %d %d %d %d %d %d\n" % (xcor.STATS[vm.stat], p0.hex(), p1.hex(), vm.nlag, vm.nexp, trail.shape[2], vm.nkp, vm.nvsys,
                                                  vm.offset is not None))
        for x in (trail, vm.lag_kms, vm.kp, vm.vsys, vm.orbit) + ((vm.offset,) if vm.offset is not None else ()):
            f.write(hexes(x) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    words = out.stdout.split()
    rows, cells = vm.nlag * vm.nexp, vm.nkp * vm.nvsys
    assert len(words) == rows + cells + 2 and words[0] == "per" and words[rows + 1] == "map"
    val = lambda ws: np.array([float.fromhex(w) for w in ws])
    return val(words[1:rows + 1]).reshape(vm.nlag, vm.nexp), val(words[rows + 2:]).reshape(vm.nkp, vm.nvsys)


@pytest.mark.parametrize("nexp,nseg,offset", [(7, 8, False), (7, 70, True), (100, 40, True)])
def test_kernel_arithmetic_on_exact_buffers_under_sanitizers(check_exe, tmp_path, nexp, nseg, offset):
    """More than 64 segments and more than 64 exposures take a second trip of the kernels' loops."""
    rng = np.random.default_rng(nexp + nseg)
    trail = random_trail(rng, 55, nexp, nseg)
    trail[:, :, 1] = 0.0                                                 # an empty segment
    for stat in STATS:
        vm = the_map(stat, nexp, offset)
        per, m = run_check(check_exe, tmp_path / "in.txt", trail, vm)
        want = xcor.trail_statistic(trail, vm)
        assert np.array_equal(m, xcor.map_from_per(per, vm), equal_nan=True), stat
        assert np.count_nonzero(np.isnan(m)) == 7 and not np.any(np.isnan(per))
        if stat == "loglike_bl19":
            ratio = np.abs(per - want) / xcor.per_bound(trail, vm)
            print("loglike_bl19: %d of %d rows differ from numpy, worst / per_bound %.4f" % (np.count_nonzero(per != want), per.size, ratio.max()))
            assert ratio.max() <= 1.0
        else:
            assert np.array_equal(per, want), stat


def test_hand_worked_cases_through_the_kernel_arithmetic(check_exe, tmp_path):
    vm = xcor.VelocityMap([-1.0, 1.0], [0.5], [0.0], [1.0, -1.0])
    per, m = run_check(check_exe, tmp_path / "a.txt", hand_trail(), vm)
    assert np.array_equal(per, xcor.trail_statistic(hand_trail(), vm)) and not np.signbit(per[0, 1])
    assert np.array_equal(m, xcor.map_from_per(per, vm))
    one = xcor.VelocityMap([5.0], [1.0], [5.0, 5.5], [0.0, 0.0])
    per, m = run_check(check_exe, tmp_path / "b.txt", np.stack([ORDINARY, OTHER]).reshape(1, 2, 1, 7), one)
    assert np.array_equal(m, [[xcor.ccf(ORDINARY) + xcor.ccf(OTHER), np.nan]], equal_nan=True)
    edge = xcor.VelocityMap([0.0, 2.0, 4.0], [10.0], [2.0, 4.0, np.nextafter(4.0, np.inf), np.nextafter(0.0, -np.inf)], [0.0], stat="chi2", a=0.0, b=0.0)
    trail = np.zeros((3, 1, 1, 7))
    trail[:, 0, 0, 6] = [1.0, 3.0, 7.0]                                  # chi2 with a = b = 0 is m6
    per, m = run_check(check_exe, tmp_path / "c.txt", trail, edge)
    assert np.array_equal(per, [[1.0], [3.0], [7.0]]) and np.array_equal(m, [[3.0, 7.0, np.nan, np.nan]], equal_nan=True)
