"""The Kp-Vsys map under the exposure table (trx_run_exposed_map) without a device: transit_amd.xcor's definitions
(exposed_map_rows, exposed_map_reference) against cases worked by hand and against filtered_map_reference, and the host
side the library compiles -- exposed_map_checks, the spans, bases and row arrays, the index -> row transform and
exposed_map_extents (transit_amd/csrc/trx_expmap.h) -- on the CPU through tests/expmap_check.cpp, a stand-alone program
over exact-size buffers under -fsanitize=address,undefined."""
import os
import subprocess

import numpy as np
import pytest

from host_check import build_check

import xcor_checks as xc
from transit_amd import _abi, xcor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = (2 ** 31 - 1, -1)


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("expmap_check", tmp_path_factory.mktemp("expmap_check"))


def test_refusals_rows_and_extents_under_sanitizers(check_exe):
    """every refusal's code and text; spans, bases, R and the row arrays for one cell, an exposure without a span, all cells
    outside, a span of one lag and nlag = 1; the index -> row transform walked over exact-size buffers; the extents at a
    small cap, at the cap and above it"""
    out = subprocess.run([check_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == ""                              # (no sanitizer report)
    lines = out.stdout.splitlines()
    last = lines[-1].split()
    assert last[0] == "ok" and int(last[1]) > 300, lines[-20:]
    assert not [line for line in lines if line.startswith("FAILED")]


def test_the_pair_cap_is_mirrored():
    txt = open(os.path.join(ROOT, "transit_amd", "csrc", "hip", "trx_device.h")).read()
    cap = _abi.EXPOSED_MAP_PAIR_BYTES
    assert cap == 2 ** 33 and cap & (cap - 1) == 0
    assert "constexpr uint64_t kExposedMapPairBytes = (uint64_t)1 << %d;" % (cap.bit_length() - 1) in txt


def rows_of_the_program(exe, path, vm):
    hexes = lambda x: " ".join(float(v).hex() for v in np.asarray(x, dtype=np.float64).ravel())
    with open(path, "w") as f:
        f.write("%d %d %d %d %d\n" % (vm.nlag, vm.nkp, vm.nvsys, vm.nexp, vm.offset is not None))
        f.write("\n".join(hexes(x) for x in (vm.lag_kms, vm.kp, vm.vsys, vm.orbit) + ((vm.offset,) if vm.offset is not None else ())) + "\n")
    out = subprocess.run([exe, "rows", str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-4000:]
    w = [int(x) for x in out.stdout.split()]
    t = np.array(w[:-1], dtype=np.int64).reshape(vm.nexp, 3)
    return t[:, 0], t[:, 1], t[:, 2], w[-1]


def same_rows(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_exposed_map_rows_by_hand():
    # test_cellmap_host's map: (Kp 1, Vsys 0) takes the lags (1, 0), (Kp 0, Vsys 0) the lags (0, 0); the two others are outside
    vm = xcor.VelocityMap([-1.0, 1.0], [1.0, 0.0], [0.0, 1.5], [1.0, -1.0])
    lo, hi, base, R = xcor.exposed_map_rows(vm)
    assert (lo.tolist(), hi.tolist(), base.tolist(), R) == ([0, 0], [1, 0], [0, 2], 3)
    # one cell: a span of one lag at every exposure
    one = xcor.VelocityMap([-1.0, 1.0], [1.0], [0.0], [1.0, -1.0])
    lo, hi, base, R = xcor.exposed_map_rows(one)
    assert (lo.tolist(), hi.tolist(), base.tolist(), R) == ([1, 0], [1, 0], [0, 1], 2)
    # every cell outside: no row
    none = xcor.VelocityMap([-1.0, 1.0], [1.0, 0.0], [1.5, 9.0], [1.0, -1.0])
    lo, hi, base, R = xcor.exposed_map_rows(none)
    assert (lo.tolist(), hi.tolist(), base.tolist(), R) == ([EMPTY[0]] * 2, [EMPTY[1]] * 2, [0, 0], 0)
    # one lag: lag 0 or outside
    single = xcor.VelocityMap([6.0], [0.0], [6.0, 7.0], [0.5, 0.25, 0.0])
    lo, hi, base, R = xcor.exposed_map_rows(single)
    assert (lo.tolist(), hi.tolist(), base.tolist(), R) == ([0] * 3, [0] * 3, [0, 1, 2], 3)


def test_exposed_map_rows_is_the_programs(check_exe, tmp_path):
    vms = [xcor.VelocityMap([-1.0, 1.0], [1.0, 0.0], [0.0, 1.5], [1.0, -1.0]),
           xcor.VelocityMap([-1.0, 1.0], [1.0, 0.0], [1.5, 9.0], [1.0, -1.0]),
           xcor.VelocityMap([6.0], [0.0], [6.0, 7.0], [0.5, 0.25, 0.0])]
    rng = np.random.default_rng(23)
    for k in range(12):
        nlag, nkp, nvsys, nexp = int(rng.integers(1, 60)), int(rng.integers(1, 15)), int(rng.integers(1, 12)), int(rng.integers(1, 9))
        kms = np.cumsum(rng.uniform(0.5, 4.0, nlag)) - rng.uniform(20.0, 60.0)
        # (spans that reach over the grid's ends: some cells outside, in some maps all of them)
        reach = (kms[-1] - kms[0] + 4.0) * (0.2 if k % 4 else 1.5)
        away = 1e4 if k in (5, 9) else 0.0                                # (two maps far above the grid: every cell outside)
        vms.append(xcor.VelocityMap(kms, rng.uniform(0.0, reach, nkp), away + rng.uniform(kms[0] - 1.0, kms[-1] + 1.0, nvsys), np.sin(rng.uniform(0.0, 6.3, nexp)),
                                    offset=rng.normal(0.0, 0.3, nexp) if k % 2 else None))
    some_outside = all_outside = 0
    for n, vm in enumerate(vms):
        want = xcor.exposed_map_rows(vm)
        assert same_rows(rows_of_the_program(check_exe, tmp_path / ("m%d.txt" % n), vm), want), n
        lo, hi, base, R = want
        idx = xcor.nearest_lags(vm).reshape(-1, vm.nexp)
        inside = np.all(idx >= 0, axis=1)
        some_outside += bool(np.any(~inside) and np.any(inside))
        all_outside += not np.any(inside)
        assert R == int(np.sum(np.maximum(hi - lo + 1, 0))) and (R == 0) == (not np.any(inside))
        if np.any(inside):
            # every inside cell's row lies inside [0, R), and two different (lag, exposure) pairs never share one
            r = base[None, :] + idx[inside] - lo[None, :]
            assert r.min() >= 0 and r.max() < R
            pairs = {(int(rr), int(l), v) for row, lags in zip(r, idx[inside]) for v, (rr, l) in enumerate(zip(row, lags))}
            assert len({p[0] for p in pairs}) == len(pairs)
    assert some_outside >= 3 and all_outside >= 2


def exposed(pairs, scale):
    """pairs_lv [nlag, nexp, npix, 2] of lag pairs [nlag, npix, 2] under a table of scales alone: a is scale[v] * a"""
    out = np.repeat(np.asarray(pairs, dtype=np.float64)[:, None], len(scale), axis=1)
    out[..., 0] = np.asarray(scale, dtype=np.float64)[None, :, None] * out[..., 0]
    return out


def test_exposed_map_reference_by_hand():
    pairs, obs, filt = xc.hand_case()
    vm = xcor.VelocityMap([-1.0, 1.0], [1.0, 0.0], [0.0, 1.5], [1.0, -1.0], stat="chi2", a=1.0, b=0.0)
    m = xcor.exposed_map_reference(exposed(pairs, (1.0, 0.0)), obs, filt, vm)
    # the model is 0 at exposure 1, live where it was.
    # cell (Kp 1, Vsys 0): M = (lag 1, 0 x lag 0) = ((2, dead, 1, 5), (0, 0, 0, 0)); column 1 is dead in this cell.
    #   segment 0, pixel 0: c = 1, g' = (1, -1): (1 - 1)^2 = 0 and (0 + 1)^2 = 1
    #   segment 1: g'[0] = (1, 5), g'[1] = (0, 0) - (1, 5): (2-1)^2 + (4-5)^2 = 2 and (1+1)^2 + (3+5)^2 = 68
    # cell (Kp 0, Vsys 0): M = (lag 0, 0 x lag 0) = ((1, 2, 3, 4), (0, 0, 0, 0)), every column live.
    #   segment 0: c = (0.5, 1), g' = ((0.5, 1), (-0.5, -1)): 0.25 + 1 = 1.25 and 0.25 + 9 = 9.25
    #   segment 1: g'[0] = (3, 4), g'[1] = -(3, 4): 1 + 0 = 1 and 16 + 49 = 65
    assert np.array_equal(m, [[71.0, np.nan], [76.5, np.nan]], equal_nan=True)
    # the cell through its parts
    M = exposed(pairs, (1.0, 0.0))[[1, 0], [0, 1]]
    val = xcor.filter_reference(M, obs, filt)
    assert np.array_equal(val, [[1.0, np.nan, 1.0, 5.0], [-1.0, np.nan, -1.0, -5.0]], equal_nan=True)
    assert xcor.cell_value(xcor.reference_values(val, obs), vm) == 71.0
    with pytest.raises(ValueError):
        xcor.exposed_map_reference(pairs, obs, filt, vm)                          # the lag pairs, without the exposure axis
    with pytest.raises(ValueError):
        xcor.exposed_map_reference(exposed(pairs, (1.0,)), obs, filt, vm)


@pytest.mark.parametrize("stat", ("ccf", "loglike_bl19", "chi2"))
@pytest.mark.parametrize("kind", ("plain", "weighted", "highpass"))
def test_pairs_repeated_over_the_exposures_give_the_filtered_map(stat, kind):
    rng = np.random.default_rng(5)
    nlag, nexp, npix = 9, 5, 40
    kms = np.cumsum(rng.uniform(1.0, 3.0, nlag)) - 9.0
    pairs = np.stack([rng.normal(1.0, 0.3, (nlag, npix)), rng.uniform(0.5, 1.5, (nlag, npix))], axis=-1)
    pairs[2, 7] = 0.0                                                    # dead at lag 2 only
    obs = xcor.Observed(xcor.segments([1, 17, 0, 22]), rng.normal(1.0, 0.3, (nexp, npix)), weight=rng.uniform(0.0, 2.0, (nexp, npix)),
                        gain=rng.uniform(0.9, 1.1, npix))
    filt = xcor.svd_filter(obs.data, obs.seg_first, 2)
    if kind == "weighted":
        filt = xcor.WeightedFilter(xcor.svd_basis(obs.data, obs.seg_first, 2))
    vm = xcor.VelocityMap(kms, [2.0, 6.0, 40.0], np.linspace(-6.0, 6.0, 5), np.sin(np.linspace(-1.0, 1.0, nexp)), stat=stat, scale=0.9, a=1.1, b=0.2)
    inside = np.all(xcor.nearest_lags(vm) >= 0, axis=-1)
    assert np.any(inside) and np.any(~inside)
    pairs_lv = exposed(pairs, np.ones(nexp))
    if kind == "highpass":
        hp = xcor.boxcar_highpass(5)
        free = xcor.Observed(obs.seg_first, obs.data, obs.weight)
        want = xcor.filtered_map_reference(xcor.highpass_pairs(xcor.highpass_reference(pairs, obs, hp)), free, filt, vm)
        got = xcor.exposed_map_reference(pairs_lv, obs, filt, vm, hp=hp)
    else:
        want = xcor.filtered_map_reference(pairs, obs, filt, vm)
        got = xcor.exposed_map_reference(pairs_lv, obs, filt, vm)
    assert np.array_equal(np.isnan(got), ~inside) and np.array_equal(got, want, equal_nan=True)
    # and a scale that is not 1 moves every inside cell
    other = xcor.exposed_map_reference(exposed(pairs, np.linspace(0.0, 1.0, nexp)), obs, filt, vm, hp=hp if kind == "highpass" else None)
    assert np.array_equal(np.isnan(other), ~inside) and np.all(other[inside] != got[inside])
