"""Band integrals on the device (trx_set_bands / trx_run_bands and the batch forms, include/transit_hip.h).

A band run must leave the spectrum exactly as trx_run computes it, and return per band the pair
(sum of w_i S_i, sum of w_i) over the shard's bins: checked against math.fsum over the returned spectrum with the
header's range rule, for bit reproducibility (repeats, with and without the spectrum, inside a larger set, through a
batch) and over shards combined in rank order."""
import ctypes as C
import math
import os
import shutil

import numpy as np
import pytest

import pixel_cases as pc
from cases import GOLDEN
from transit_amd import _abi, bands
from transit_amd.engine import Batch, Engine, EngineError
from transit_amd.host import Problem

pytestmark = pytest.mark.gpu


def reference(P, bs, spec, lo=0):
    """math.fsum of the band sums over the spectrum of shard [lo, lo + len(spec))"""
    ref = np.zeros((len(bs), 2))
    for k, b in enumerate(bs):
        i, w = pc.band_bins(P, b)
        m = (i >= lo) & (i < lo + spec.size)
        ref[k, 0] = math.fsum(w[m] * spec[i[m] - lo])
        ref[k, 1] = math.fsum(w[m])
    return ref


def check_accuracy(P, bs, sums, spec, lo=0):
    ref = reference(P, bs, spec, lo)
    for k, b in enumerate(bs):
        tol = 1e-12 if b.kind == _abi.BAND_GAUSS else 1e-13
        for c in range(2):
            r, g = ref[k, c], sums[k, c]
            if r == 0:
                assert g == 0, (k, c, g)
            else:
                assert abs(g - r) <= tol * abs(r), (k, c, g, r, abs(g - r) / abs(r))


@pytest.mark.parametrize("solution", ["eclipse", "transit"])
def test_band_runs_keep_the_spectrum_and_sum_it(tmp_path, solution):
    P = pc.make_band_case(tmp_path, solution)
    bs = pc.band_set(P)
    plain, banded = Engine(P.static), Engine(P.static)
    banded.set_bands(bs)
    deep, keep = pc.thinner(P, 1e-3)
    for atm in (P.atm, P.atm, deep, P.atm):        # fresh, hinted, resuming deeper, hinted again
        ref = plain.run(atm, P.opts)["spectrum"]
        sums, spec = banded.run_bands(atm, P.opts, spectrum=True)
        assert np.array_equal(spec, ref)
        check_accuracy(P, bs, sums, spec)
    assert plain.stats()["layers_swept"] > 0
    # trx_run on a handle with bands installed: the plain spectrum
    for atm in (P.atm, deep):
        assert np.array_equal(banded.run(atm, P.opts)["spectrum"], plain.run(atm, P.opts)["spectrum"])
    # bit reproducibility: repeats, with and without the spectrum, the set inside a larger one
    first = banded.run_bands(P.atm, P.opts)
    for _ in range(2):
        assert np.array_equal(banded.run_bands(P.atm, P.opts), first)
    assert np.array_equal(banded.run_bands(P.atm, P.opts, spectrum=True)[0], first)
    extra = bands.resolving_power(np.linspace(2510.5, 2890.5, 50), 1000.0) + [bands.weights(0, np.ones(P.nwn))]
    banded.set_bands(extra + bs)
    assert np.array_equal(banded.run_bands(P.atm, P.opts)[len(extra):], first)
    plain.close(); banded.close()


def test_batch_band_sums_are_the_single_handle_sums(tmp_path):
    P = pc.make_band_case(tmp_path, "eclipse", nlines=120_000, seed=33)
    bs = pc.band_set(P, seed=3)
    K = 11
    atms, keep = pc.atmospheres(P, K)
    one = Engine(P.static)
    one.set_bands(bs)
    ref = np.stack([one.run_bands(atms[j], P.opts) for j in range(K)])
    one.close()
    assert len({ref[j].tobytes() for j in range(K)}) == K
    B = Batch(P.static, ways=3)
    B.set_bands(bs)
    for rep in range(3):
        got = B.run_bands(atms, P.opts)
        assert got.shape == (K, len(bs), 2)
        assert np.array_equal(got, ref), rep
    B.close()


@pytest.mark.parametrize("solution", ["eclipse", "transit"])
def test_shards_combined_in_rank_order(tmp_path, solution):
    P = pc.make_band_case(tmp_path, solution, nlines=60_000, nlayers=80)
    bs = pc.band_set(P, seed=5)
    n = P.nwn
    whole = Engine(P.static)
    whole.set_bands(bs)
    total, spec = whole.run_bands(P.atm, P.opts, spectrum=True)
    whole.close()
    check_accuracy(P, bs, total, spec)
    cuts = [0, 90, 251, n]
    parts = []
    try:
        for r in range(3):
            P.set_shard(cuts[r], cuts[r + 1])
            E = Engine(P.static)
            E.set_bands(bs)
            s, sp = E.run_bands(P.atm, P.opts, spectrum=True)
            E.close()
            check_accuracy(P, bs, s, sp, lo=cuts[r])
            for k, b in enumerate(bs):
                i, _ = pc.band_bins(P, b)
                if not np.any((i >= cuts[r]) & (i < cuts[r + 1])):
                    assert s[k, 0] == 0 and s[k, 1] == 0 and not np.signbit(s[k, 0]), (r, k)
            parts.append(s)
    finally:
        P.set_shard(0, n)
    got = bands.combine(parts)
    ok = total != 0
    assert np.all(got[~ok] == 0)
    assert np.max(np.abs(got[ok] - total[ok]) / np.abs(total[ok])) <= 1e-12


def test_large_grid_many_gaussians(tmp_path):
    """above kEmisRowsAbove bins (k_emission_rows): 10^4 Gaussians at R = 3000, bands of many pieces"""
    P = pc.make_band_case(tmp_path, "eclipse", nlines=100_000, wnlow=2500, wnhigh=2800, wndelt=0.001, wnosamp=1, nlayers=60)
    wn_i, wn_d, n, wn = pc.grid(P)
    assert n > 65536 and n >= 3 * 10 ** 5
    bs = bands.resolving_power(np.linspace(wn[0] + 1.0, wn[-1] - 1.0, 10_000), 3000.0)
    bs += [bands.weights(0, 1.0 + 0.25 * np.cos(np.arange(n) * 1e-3)), bands.tophat(wn, 2600.0, 2700.0),
           bands.gauss(2650.0, 20.0, 6.0)]
    plain, banded = Engine(P.static), Engine(P.static)
    banded.set_bands(bs)
    for _ in range(2):
        ref = plain.run(P.atm, P.opts)["spectrum"]
        sums, spec = banded.run_bands(P.atm, P.opts, spectrum=True)
        assert np.array_equal(spec, ref)
        check_accuracy(P, bs, sums, spec)
    assert np.array_equal(banded.run_bands(P.atm, P.opts), sums)
    plain.close(); banded.close()


def test_opacity_grid_handle(tmp_path):
    d = tmp_path / "og"
    shutil.copytree(os.path.join(GOLDEN, "opacity_grid"), d)
    P = Problem.from_cfg(os.path.join(str(d), "case.cfg"))
    builder = Engine(P.static)
    builder.build_opacity_grid(P)
    builder.close()
    assert P.static.ogrid
    bs = pc.band_set(P, seed=7)
    plain, banded = Engine(P.static), Engine(P.static)
    banded.set_bands(bs)
    for _ in range(2):
        ref = plain.run(P.atm, P.opts)["spectrum"]
        sums, spec = banded.run_bands(P.atm, P.opts, spectrum=True)
        assert np.array_equal(spec, ref)
        check_accuracy(P, bs, sums, spec)
        assert np.array_equal(banded.run(P.atm, P.opts)["spectrum"], ref)
    plain.close(); banded.close()


def test_refusals_keep_the_previous_set(tmp_path):
    P = pc.make_band_case(tmp_path, "eclipse", nlines=20_000, wnhigh=2600, nlayers=60)
    n = P.nwn
    E = Engine(P.static)
    with pytest.raises(EngineError) as ei:             # no set installed
        E.run_bands(P.atm, P.opts)
    assert ei.value.code == -1
    good = [bands.weights(0, np.ones(n)), bands.gauss(2550.0, 2.0)]
    E.set_bands(good)
    before = E.run_bands(P.atm, P.opts)
    bad = {
        "unknown kind": bands.Band(kind=7),
        "n < 1": bands.weights(3, []),
        "first < 0": bands.weights(-1, [1.0]),
        "first + n > nwn": bands.weights(n - 1, [1.0, 1.0]),
        "not finite": bands.weights(0, [1.0, np.nan]),
        "not finite ": bands.weights(0, [np.inf]),
        "fwhm <= 0": bands.gauss(2550.0, 0.0),
        "fwhm <= 0 ": bands.gauss(2550.0, -1.0),
        "cut <= 0": bands.gauss(2550.0, 1.0, 0.0),
        "cut <= 0 ": bands.gauss(2550.0, 1.0, -2.0),
    }
    for what, b in bad.items():
        with pytest.raises(EngineError) as ei:
            E.set_bands(good + [b])
        assert ei.value.code == -1 and "band 2" in str(ei.value), what
        assert np.array_equal(E.run_bands(P.atm, P.opts), before), what
    lib = E._lib
    arr = bands.to_c(good)
    assert lib.trx_set_bands(E._h, -1, arr) == -1
    sums = np.zeros((2, 2))
    assert lib.trx_run_bands(E._h, C.byref(P.atm), C.byref(P.opts), None, None, None) == -1
    assert lib.trx_run_bands(E._h, C.byref(P.atm), C.byref(P.opts), None,
                             sums.ctypes.data_as(_abi.c_double_p), None) == 0
    assert np.array_equal(sums, before)
    E.set_bands([])                                    # cleared: refused again
    with pytest.raises(EngineError):
        E.run_bands(P.atm, P.opts)
    E.close()
    # a batch installs a set on every handle or on none
    B = Batch(P.static, ways=2)
    with pytest.raises(EngineError):
        B.run_bands([P.atm], P.opts)
    B.set_bands(good)
    ref = B.run_bands([P.atm, P.atm, P.atm], P.opts)
    assert np.array_equal(ref[0], before) and np.array_equal(ref[2], before)
    with pytest.raises(EngineError) as ei:
        B.set_bands(good + [bands.gauss(2550.0, 1.0, 0.0)])
    assert "band 2" in str(ei.value)
    assert np.array_equal(B.run_bands([P.atm, P.atm, P.atm], P.opts), ref)
    B.close()
