"""The filtered Kp-Vsys map (trx_run_filtered_map) without a device: transit_amd.xcor's definitions (nearest_lags,
cell_value, cell_bound, filtered_map_reference) against cases worked by hand, and the host side the library compiles --
vmap_nearest (transit_amd/csrc/trx_vmap.h), filtered_map_checks and cell_map_extents (transit_amd/csrc/trx_products.h)
-- on the CPU through tests/cellmap_check.cpp, a stand-alone program over exact-size buffers under
-fsanitize=address,undefined."""
import os
import subprocess

import numpy as np
import pytest

from host_check import build_check

import xcor_checks as xc
from transit_amd import _abi, xcor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("cellmap_check", tmp_path_factory.mktemp("cellmap_check"))


def test_refusals_and_extents_under_sanitizers(check_exe):
    """every refusal's code and text; the extents for one cell, the cap, cap + 1 and a byte cap that forces one cell a chunk,
    walked over exact-size buffers"""
    out = subprocess.run([check_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == ""                              # (no sanitizer report)
    lines = out.stdout.splitlines()
    last = lines[-1].split()
    assert last[0] == "ok" and int(last[1]) > 300, lines[-20:]
    assert not [line for line in lines if line.startswith("FAILED")]


def test_the_chunk_cap_is_mirrored():
    txt = open(os.path.join(ROOT, "transit_amd", "csrc", "hip", "trx_device.h")).read()
    assert "constexpr int kCellMapChunk = %d;" % _abi.CELLMAP_CHUNK in txt


def nearest_of_the_program(exe, path, kms, xs):
    hexes = lambda x: " ".join(float(v).hex() for v in np.asarray(x, dtype=np.float64).ravel())
    with open(path, "w") as f:
        f.write("%d %d\n%s\n%s\n" % (len(kms), len(xs), hexes(kms), hexes(xs)))
    out = subprocess.run([exe, "nearest", str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-4000:]
    return np.array([int(w) for w in out.stdout.split()])


def nearest_of_xcor(kms, xs):
    """xcor.nearest_lags at the velocities xs: kp = 0 and orbit = 0 leave x = vsys"""
    return xcor.nearest_lags(xcor.VelocityMap(kms, [0.0], xs, [0.0]))[0, :, 0]


def test_vmap_nearest_is_nearest_lags(check_exe, tmp_path):
    up, down = (lambda x: np.nextafter(x, np.inf)), (lambda x: np.nextafter(x, -np.inf))
    kms = np.array([-3.0, 0.0, 3.0, 7.5, 8.0, 81.0])
    mid = 0.5 * (kms[:-1] + kms[1:])                                   # exact: -1.5, 1.5, 5.25, 7.75, 44.5
    assert np.all((mid - kms[:-1]) / (kms[1:] - kms[:-1]) == 0.5)
    xs = np.concatenate([kms, mid, up(mid), down(mid), [down(kms[-1]), up(kms[0])],        # inside
                         [up(kms[-1]), down(kms[0]), 1e300, -1e300, np.inf, -np.inf, np.nan]])      # outside, or not finite
    got, want = nearest_of_the_program(check_exe, tmp_path / "a.txt", kms, xs), nearest_of_xcor(kms, xs)
    assert np.array_equal(got, want)
    n = len(kms)
    assert np.array_equal(got[:n], np.arange(n))                       # on a node: that node, the last one included
    assert np.array_equal(got[n:2 * n - 1], np.arange(n - 1))          # an exact midpoint: the tie goes to the lower lag
    assert np.array_equal(got[2 * n - 1:3 * n - 2], np.arange(1, n))   # one ulp above it: the upper
    assert np.array_equal(got[3 * n - 2:4 * n - 3], np.arange(n - 1))  # one ulp below it: the lower
    assert list(got[4 * n - 3:4 * n - 1]) == [n - 1, 0]
    assert np.all(got[4 * n - 1:] == -1)                               # one ulp outside either end, and what is not finite
    # random velocities on the GPU tests' grid, and a grid of uneven steps
    rng = np.random.default_rng(11)
    for grid in (xcor.lag_grid(-81.0, 81.0, 3.0)[0], np.cumsum(rng.uniform(0.01, 5.0, 40)) - 50.0):
        xs = rng.uniform(grid[0] - 2.0, grid[-1] + 2.0, 4000)
        got = nearest_of_the_program(check_exe, tmp_path / "b.txt", grid, xs)
        assert np.array_equal(got, nearest_of_xcor(grid, xs))
        inside = (xs >= grid[0]) & (xs <= grid[-1])
        assert np.all(got[~inside] == -1) and np.count_nonzero(~inside) > 10
        assert np.array_equal(got[inside], np.argmin(np.abs(xs[inside, None] - grid[None, :]), axis=1))      # (no random tie)
    # one lag: the lag itself, or outside
    one = np.array([6.0])
    xs = np.array([6.0, up(6.0), down(6.0), 0.0, np.nan])
    got = nearest_of_the_program(check_exe, tmp_path / "c.txt", one, xs)
    assert np.array_equal(got, nearest_of_xcor(one, xs)) and list(got) == [0, -1, -1, -1, -1]


def test_nearest_lags_of_a_map_marks_the_offending_exposures_only():
    vm = xcor.VelocityMap([-1.0, 1.0], [1.0, 0.0], [0.0, 1.5], [1.0, -1.0])
    idx = xcor.nearest_lags(vm)
    assert idx.shape == (2, 2, 2)
    # (Kp 1, Vsys 0): +1 and -1, on the nodes; (Kp 1, Vsys 1.5): 2.5 is outside, 0.5 is nearer to +1;
    # (Kp 0, Vsys 0): 0 is the midpoint, the lower lag at both exposures; (Kp 0, Vsys 1.5): outside at both
    assert idx.tolist() == [[[1, 0], [-1, 1]], [[0, 0], [-1, -1]]]
    off = xcor.VelocityMap([-1.0, 1.0], [1.0], [0.0], [1.0, -1.0], offset=[0.25, np.inf])
    assert xcor.nearest_lags(off).tolist() == [[[-1, -1]]]


def test_filtered_map_reference_by_hand():
    pairs, obs, filt = xc.hand_case()
    vm = xcor.VelocityMap([-1.0, 1.0], [1.0, 0.0], [0.0, 1.5], [1.0, -1.0], stat="chi2", a=1.0, b=0.0)
    m = xcor.filtered_map_reference(pairs, obs, filt, vm)
    # cell (Kp 1, Vsys 0): M = (lag 1, lag 0) = ((2, dead, 1, 5), (1, 2, 3, 4)); column 1 is dead in THIS cell.
    #   segment 0, pixel 0: c = 1.5, g' = (0.5, -0.5): (1 - 0.5)^2 = 0.25 and (0 + 0.5)^2 = 0.25
    #   segment 1: g'[0] = (1, 5), g'[1] = (3, 4) - (1, 5) = (2, -1): (2-1)^2 + (4-5)^2 = 2 and (1-2)^2 + (3+1)^2 = 17
    # cell (Kp 0, Vsys 0): M = (lag 0, lag 0), every column live.
    #   segment 0: g' = 0: 1 + 0 = 1 and 0 + 4 = 4;  segment 1: g'[0] = (3, 4), g'[1] = 0: 1 + 0 = 1 and 1 + 9 = 10
    assert np.array_equal(m, [[19.5, np.nan], [16.0, np.nan]], equal_nan=True)
    # the same cell through its parts: the values, the moments, points 5
    val = xcor.filter_reference(pairs[[1, 0]], obs, filt)
    assert np.array_equal(val, [[0.5, np.nan, 1.0, 5.0], [-0.5, np.nan, 2.0, -1.0]], equal_nan=True)
    mom = xcor.reference_values(val, obs)
    assert mom[:, :, 0].tolist() == [[1.0, 2.0], [1.0, 2.0]]
    assert xcor.cell_value(mom, vm) == 19.5
    # ccf skips the one-pixel rows of segment 0 (n < 2): the sum over the two rows of segment 1 alone
    cc = xcor.VelocityMap([-1.0, 1.0], [1.0], [0.0], [1.0, -1.0])
    want = float(xcor.ccf(mom[0, 1])) + float(xcor.ccf(mom[1, 1]))
    assert np.all(np.isnan(xcor.ccf(mom[:, 0]))) and xcor.cell_value(mom, cc) == want
    assert xcor.filtered_map_reference(pairs, obs, filt, cc)[0, 0] == want
    # all rows skipped: +0
    assert xcor.cell_value(mom[:, :1], cc) == 0.0
    # the bound: (c + nseg + nexp) 2^-52 times the sum of the |statistics|
    assert xcor.cell_bound(mom, vm) == (4 + 2 + 2) * EPS * 19.5
    assert xcor.cell_bound(mom, xcor.VelocityMap([-1.0, 1.0], [1.0], [0.0], [1.0, -1.0], stat="loglike_bl19")) == \
        (5 + 2 + 2) * EPS * float(np.nansum(np.abs(xcor.loglike_bl19(mom))))
    with pytest.raises(ValueError):
        xcor.filtered_map_reference(pairs[:1], obs, filt, vm)
    with pytest.raises(ValueError):
        xcor.cell_value(mom[:1], vm)


@pytest.mark.parametrize("stat", ("ccf", "loglike_bl19", "chi2"))
def test_an_all_zero_filter_on_nodes_is_the_unfiltered_map(stat):
    """orbit = 0 and every Vsys on a lag node (not the last: there map_from_per forms per[k] + 1 * (per[k+1] - per[k]),
    which rounds): the nearest lag is the track's own, the filter takes nothing out, and the cell is the sum over the
    exposures of the trail statistic at that lag -- map_from_per's bits."""
    rng = np.random.default_rng(3)
    nlag, nexp, npix = 6, 5, 40
    kms = np.array([-7.0, -3.0, 0.0, 1.0, 4.0, 9.0])
    pairs = np.stack([rng.normal(1.0, 0.3, (nlag, npix)), rng.uniform(0.5, 1.5, (nlag, npix))], axis=-1)
    pairs[2, 7] = 0.0                                                    # dead at lag 2 only
    obs = xcor.Observed(xcor.segments([1, 17, 0, 22]), rng.normal(1.0, 0.3, (nexp, npix)), weight=rng.uniform(0.0, 2.0, (nexp, npix)),
                        gain=rng.uniform(0.9, 1.1, npix))
    filt = xcor.Filter(np.zeros((4, 1, nexp)), np.zeros((4, nexp, 1)))
    vm = xcor.VelocityMap(kms, [10.0, 250.0], [kms[2], kms[0], kms[4], 8.0, 9.5], np.zeros(nexp), stat=stat, scale=0.9, a=1.1, b=0.2)
    assert xcor.nearest_lags(vm)[0, :, 0].tolist() == [2, 0, 4, 5, -1]
    m = xcor.filtered_map_reference(pairs, obs, filt, vm)
    want = xcor.map_from_per(xcor.trail_statistic(xcor.trail_reference(pairs, obs), vm), vm)
    assert np.array_equal(m[:, :3], want[:, :3]) and np.all(np.isfinite(m[:, :4])) and np.all(np.isnan(m[:, 4])) and np.all(np.isnan(want[:, 4]))
    assert np.array_equal(m[0], m[1], equal_nan=True)                    # (orbit = 0: Kp does not matter)
    # 8.0 is nearer to the last lag: the statistic at that lag, not an interpolation
    at_last = xcor.VelocityMap(kms, [10.0], [9.0], np.zeros(nexp), stat=stat, scale=0.9, a=1.1, b=0.2)
    assert m[0, 3] == xcor.filtered_map_reference(pairs, obs, filt, at_last)[0, 0] != want[0, 3]
