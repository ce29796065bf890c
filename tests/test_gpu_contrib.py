"""Contribution functions per band and layer on the device (trx_run_contrib / trx_run_batch_contrib,
include/transit_hip.h) against transit_amd.contrib, the numpy statement of the same definition.

The per-(band, layer) yardstick is the CEILING C[b][r] = sum_j |w_j| pi B_r(j) (eclipse) or sum_j |w_j| (transit):
every node weight W_i lies in [0, pi] and every transmittance in [0, 1], so an error is measured against what the
entry could be, not against entries that are legitimately 1e-30 of their row."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import oracle_lib as ol
import pixel_cases as pc
from cases import golden
from transit_amd import _abi, bands, contrib
from transit_amd.engine import Batch, Engine, EngineError

pytestmark = pytest.mark.gpu

GEOMETRIES = ["eclipse", "transit"]


def inputs(P, atm=None):
    """(wavenumbers in the Planck function's unit, angles, temperatures of atm)"""
    st, o = P.static, P.opts
    wn = (st.wn_i + np.arange(int(st.nwn)) * st.wn_d) * o.wn_fct
    angles = np.array([o.angles_deg[a] for a in range(int(o.nangles))])
    a = atm if atm is not None else P.atm
    temp = np.ctypeslib.as_array(a.temp, shape=(int(a.nlayer),)).copy()
    return wn, angles, temp


def per_bin(P, atm, out, lo=0):
    """the definition per (bin, layer) from a run's own tau / last (shard [lo, lo + n))"""
    wn, angles, temp = inputs(P, atm)
    n = out["tau"].shape[0]
    if P.opts.solution == _abi.SOL_ECLIPSE:
        return contrib.from_tau(out["tau"], out["last"], temp, wn[lo:lo + n], angles)
    return contrib.transmittance_from_tau(out["tau"], out["last"])


def ceiling_per_bin(P, atm, n, lo=0):
    wn, angles, temp = inputs(P, atm)
    if P.opts.solution == _abi.SOL_ECLIPSE:
        return math.pi * contrib.planck(wn[lo:lo + n], temp)
    return np.ones((n, temp.size))


def shard_bins(P, b, lo, n):
    """(local bins, weights) of band b inside shard [lo, lo + n)"""
    i, w = pc.band_bins(P, b)
    m = (i >= lo) & (i < lo + n)
    return i[m] - lo, w[m]


def reference(P, atm, bs, out, lo=0):
    """(rows [nbands, nlayer] by math.fsum, ceilings [nbands, nlayer]) of shard [lo, lo + n)"""
    F = per_bin(P, atm, out, lo)
    n = F.shape[0]
    ceil_bin = ceiling_per_bin(P, atm, n, lo)
    ref, ceil = np.zeros((len(bs), F.shape[1])), np.zeros((len(bs), F.shape[1]))
    for k, b in enumerate(bs):
        i, w = shard_bins(P, b, lo, n)
        ref[k] = contrib.reduce(F, i, w)
        ceil[k] = contrib.reduce(ceil_bin, i, np.abs(w))
    return ref, ceil


def check(got, ref, ceil, tol, what=""):
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(ceil > 0, err / ceil, 0.0))
    print(what, "max |CF - ref| / ceiling = %.3g" % worst)
    bad = np.argwhere(err > tol * ceil)
    assert bad.size == 0, (what, bad[:5], worst)


def debug_run(E, atm, opts):
    return E.run(atm, opts, debug=("tau", "last"))


def sequence(P):
    deep, keep = pc.thinner(P, 1e-3)
    return [("fresh", P.atm), ("hinted", P.atm), ("deeper", deep), ("hinted again", P.atm)], keep


@pytest.mark.parametrize("solution", GEOMETRIES)
def test_own_optical_depths_closure_and_untouched_run(tmp_path, solution):
    """tests 5, 6, 8 and 9 (a)-(c) of the issue on the band tests' problem and band set"""
    P = pc.make_band_case(tmp_path, solution)
    bs = pc.band_set(P)
    n, nl = P.nwn, P.nlayer
    dbg, plain, E = Engine(P.static), Engine(P.static), Engine(P.static)
    plain.set_bands(bs)
    E.set_bands(bs)
    seq, keep = sequence(P)
    off_grid = len(bs) - 1
    for what, atm in seq:
        out = debug_run(dbg, atm, P.opts)
        ref, ceil = reference(P, atm, bs, out)
        sums, cf, spec = E.run_contrib(atm, P.opts, spectrum=True)
        assert cf.shape == (len(bs), nl)
        # 5: against the definition on the run's own optical depths
        check(cf, ref, ceil, 1e-12, "%s %s:" % (solution, what))
        # 8: spectrum and sums are trx_run_bands'
        sums_b, spec_b = plain.run_bands(atm, P.opts, spectrum=True)
        assert np.array_equal(spec, spec_b) and np.array_equal(sums, sums_b), what
        # 6: closure on the device
        assert np.all(cf >= 0), what
        assert np.all(cf[off_grid] == 0) and not np.any(np.signbit(cf[off_grid])), what
        if solution == "eclipse":
            tot = cf.sum(axis=1)
            have = sums[:, 0] != 0
            gap = np.abs(tot[have] - sums[have, 0]) / sums[have, 0]
            print(solution, what, "closure: max |sum_r CF - sums| / sums = %.3g" % gap.max())
            assert np.all(np.abs(tot - sums[:, 0]) <= 1e-12 * sums[:, 0]), what
        else:
            for k, b in enumerate(bs):
                if sums[k, 1] == 0:
                    assert np.all(cf[k] == 0)
                    continue
                t = cf[k] / sums[k, 1]
                assert np.all((t >= 0) & (t <= 1 + 1e-12)), (what, k)
                assert t[nl - 1] >= t[0], (what, k)
                i, _ = shard_bins(P, b, 0, n)
                deepest = int(out["last"][i].max())
                assert np.all(cf[k, :nl - 1 - deepest] == 0), (what, k)
    # 8: after contribution runs the handle's run and run_bands still give their bits
    for what, atm in seq[1:3]:
        assert np.array_equal(E.run(atm, P.opts)["spectrum"], plain.run(atm, P.opts)["spectrum"]), what
        assert np.array_equal(E.run_bands(atm, P.opts), plain.run_bands(atm, P.opts)), what
    # 9 (a), (b): repeats, with and without the spectrum
    first = E.run_contrib(P.atm, P.opts)[1]
    for _ in range(2):
        assert np.array_equal(E.run_contrib(P.atm, P.opts)[1], first)
    assert np.array_equal(E.run_contrib(P.atm, P.opts, spectrum=True)[1], first)
    # 9 (c): a band alone, and the set inside a larger one
    extra = bands.resolving_power(np.linspace(2510.5, 2890.5, 50), 1000.0) + [bands.weights(0, np.ones(n))]
    E.set_bands(extra + bs)
    assert np.array_equal(E.run_contrib(P.atm, P.opts)[1][len(extra):], first)
    for k in (3, 17, 20, len(bs) - 4, len(bs) - 3):
        E.set_bands([bs[k]])
        assert np.array_equal(E.run_contrib(P.atm, P.opts)[1][0], first[k]), k
    for e in (dbg, plain, E):
        e.close()


@pytest.mark.parametrize("solution", GEOMETRIES)
def test_one_order_of_summation_across_run_forms(tmp_path, solution):
    """test 9 (d), (e): the rows do not depend on the kernels that made the optical depths or on the step plan"""
    P = pc.make_band_case(tmp_path, solution)
    bs = pc.band_set(P)
    seq, keep = sequence(P)

    def rows(E):
        E.set_bands(bs)
        return [E.run_contrib(atm, P.opts)[1] for _, atm in seq]

    E = Engine(P.static)
    ref = rows(E)
    for switch in ("TRX_RAY_TAIL", "TRX_TWO_QUEUES"):
        os.environ[switch] = "0"
        try:
            X = Engine(P.static)
        finally:
            os.environ.pop(switch, None)
        got = rows(X)
        X.close()
        for a, b, (what, _) in zip(got, ref, seq):
            assert np.array_equal(a, b), (switch, what)
    o = P.opts
    was = int(o.layer_chunk)
    try:
        for chunk in (0, 7, 64):
            o.layer_chunk = chunk
            X = Engine(P.static)
            X.set_bands(bs)
            got = [X.run_contrib(atm, o)[1] for _, atm in seq]
            X.close()
            for a, b, (what, _) in zip(got, ref, seq):
                assert np.array_equal(a, b), (chunk, what)
    finally:
        o.layer_chunk = was
    E.close()


@pytest.mark.parametrize("solution", GEOMETRIES)
def test_batch_rows_are_the_single_handle_rows(tmp_path, solution):
    """test 9 (f)"""
    P = pc.make_band_case(tmp_path, solution, nlines=60_000, seed=33)
    bs = pc.band_set(P, seed=3)
    K = 8
    atms, keep = pc.atmospheres(P, K)
    one = Engine(P.static)
    one.set_bands(bs)
    pairs = [one.run_contrib(atms[j], P.opts) for j in range(K)]
    one.close()
    ref_s, ref_c = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    assert len({ref_c[j].tobytes() for j in range(K)}) == K
    B = Batch(P.static, ways=3)
    with pytest.raises(EngineError):                   # no set installed
        B.run_contrib(atms, P.opts)
    B.set_bands(bs)
    for rep in range(2):
        s, c = B.run_contrib(atms, P.opts)
        assert c.shape == (K, len(bs), P.nlayer)
        assert np.array_equal(s, ref_s) and np.array_equal(c, ref_c), rep
    assert np.array_equal(B.run_bands(atms, P.opts), ref_s)
    B.close()


@pytest.mark.parametrize("name", ["eclipse_small", "multi_species", "transit_small", "cloud_scatter"])
def test_against_the_oracle_on_goldens(name):
    """test 7: one-bin bands over every bin against the definition on the ORACLE's optical depths, 1e-9 x ceiling
    (the suite holds the device's tau to 1e-9 relative on these cases; |d exp(-x)| <= x exp(-x) 1e-9 <= 1e-9 / e)"""
    P = golden(name).problem
    n, nl = P.nwn, P.nlayer
    ora = ol.OracleEngine(P.static)
    ref_out = ora.run(P.atm, P.opts, debug=True)
    ora.close()
    F = per_bin(P, P.atm, ref_out)
    ceil = ceiling_per_bin(P, P.atm, n)
    E = Engine(P.static)
    E.set_bands([bands.weights(j, [1.0]) for j in range(n)])
    for what in ("fresh", "hinted"):
        sums, cf = E.run_contrib(P.atm, P.opts)
        assert cf.shape == (n, nl)
        check(cf, F, ceil, 1e-9, "%s %s:" % (name, what))
    E.close()


@pytest.mark.parametrize("solution", GEOMETRIES)
def test_shards_combined_in_rank_order(tmp_path, solution):
    """test 10"""
    P = pc.make_band_case(tmp_path, solution, nlines=60_000, nlayers=80)
    bs = pc.band_set(P, seed=5)
    n = P.nwn
    dbg, whole = Engine(P.static), Engine(P.static)
    out = debug_run(dbg, P.atm, P.opts)
    dbg.close()
    _, ceil = reference(P, P.atm, bs, out)
    whole.set_bands(bs)
    total = whole.run_contrib(P.atm, P.opts)[1]
    whole.close()
    cuts = [0, n // 3, 2 * n // 3 + 5, n]
    parts = []
    try:
        for r in range(3):
            P.set_shard(cuts[r], cuts[r + 1])
            E = Engine(P.static)
            E.set_bands(bs)
            cf = E.run_contrib(P.atm, P.opts)[1]
            E.close()
            for k, b in enumerate(bs):
                i, _ = pc.band_bins(P, b)
                if not np.any((i >= cuts[r]) & (i < cuts[r + 1])):
                    assert np.all(cf[k] == 0) and not np.any(np.signbit(cf[k])), (r, k)
            parts.append(cf)
    finally:
        P.set_shard(0, n)
    check(contrib.combine(parts), total, ceil, 1e-13, "%s shards:" % solution)


def test_refusals_and_a_change_of_nlayer(tmp_path):
    """test 11"""
    P = pc.make_band_case(tmp_path / "a", "eclipse", nlines=20_000, wnhigh=2600, nlayers=60)
    Q = pc.make_band_case(tmp_path / "b", "eclipse", nlines=20_000, wnhigh=2600, nlayers=90)      # the same lines, another atmosphere
    n = P.nwn
    assert Q.nwn == n and Q.nlayer != P.nlayer
    E = Engine(P.static)
    with pytest.raises(EngineError) as ei:             # no set installed
        E.run_contrib(P.atm, P.opts)
    assert ei.value.code == -1 and "band set" in str(ei.value)
    bs = [bands.weights(0, np.ones(n)), bands.gauss(2550.0, 2.0), bands.weights(n // 2, [0.7])]
    E.set_bands(bs)
    lib = E._lib
    sums, cf = np.zeros((3, 2)), np.zeros((3, P.nlayer))
    ps, pcf = sums.ctypes.data_as(_abi.c_double_p), cf.ctypes.data_as(_abi.c_double_p)
    lib.trx_last_error.argtypes, lib.trx_last_error.restype = [C.c_void_p], C.c_char_p
    assert lib.trx_run_contrib(E._h, C.byref(P.atm), C.byref(P.opts), None, ps, None, None) == -1
    assert b"contrib" in lib.trx_last_error(E._h)
    assert lib.trx_run_contrib(E._h, C.byref(P.atm), C.byref(P.opts), None, None, pcf, None) == -1
    assert b"sums" in lib.trx_last_error(E._h)
    assert lib.trx_run_contrib(E._h, C.byref(P.atm), C.byref(P.opts), None, ps, pcf, None) == 0      # still runs
    dbg = Engine(P.static)
    # atmospheres of different nlayer one after the other on the same handles: rows of the new length
    for what, X in (("60 layers", P), ("90 layers", Q), ("60 layers again", P)):
        out = debug_run(dbg, X.atm, X.opts)
        ref, ceil = reference(X, X.atm, bs, out)
        s, c = E.run_contrib(X.atm, X.opts)
        assert c.shape == (3, X.nlayer)
        check(c, ref, ceil, 1e-12, what + ":")
        if what == "60 layers":
            assert np.array_equal(c, cf) and np.array_equal(s, sums)
    E.set_bands([])                                    # cleared: refused again
    with pytest.raises(EngineError):
        E.run_contrib(P.atm, P.opts)
    E.close(); dbg.close()


@pytest.mark.parametrize("solution", GEOMETRIES)
def test_large_grid_many_pieces(tmp_path, solution):
    """test 12: more than 64 pieces per band, the k_emission_rows side of the spectrum kernels"""
    P = pc.make_band_case(tmp_path, solution, nlines=10_000, wnlow=2500, wnhigh=2800, wndelt=0.004, wnosamp=1, nlayers=60)
    wn_i, wn_d, n, wn = pc.grid(P)
    nl = P.nlayer
    assert n >= 70_000 and n > 64 * 1024
    bs = [bands.weights(0, 1.0 + 0.25 * np.cos(np.arange(n) * 1e-3))]
    bs += bands.resolving_power(np.linspace(wn[0] + 2.0, wn[-1] - 2.0, 50), 300.0)
    dbg, E = Engine(P.static), Engine(P.static)
    E.set_bands(bs)
    out = debug_run(dbg, P.atm, P.opts)
    dbg.close()
    F = per_bin(P, P.atm, out)
    ceil_bin = ceiling_per_bin(P, P.atm, n)
    rng = np.random.default_rng(12)
    pairs = [(0, r) for r in range(nl)] + [(int(rng.integers(1, len(bs))), int(rng.integers(0, nl))) for _ in range(200)]
    for what in ("fresh", "hinted"):
        sums, cf = E.run_contrib(P.atm, P.opts)
        worst = 0.0
        for k, r in pairs:
            i, w = shard_bins(P, bs[k], 0, n)
            ref = math.fsum(w * F[i, r])
            ceil = math.fsum(np.abs(w) * ceil_bin[i, r])
            worst = max(worst, abs(cf[k, r] - ref) / ceil)
            assert abs(cf[k, r] - ref) <= 1e-12 * ceil, (what, k, r, cf[k, r], ref, ceil)
        print(solution, what, "large grid: max |CF - ref| / ceiling = %.3g" % worst)
    assert np.array_equal(E.run_contrib(P.atm, P.opts)[1], cf)
    E.close()
