"""Rotational broadening of the spectrum on the device (trx_set_broadening / trx_run_broadened and the batch forms,
include/transit_hip.h) against transit_amd.broaden, the numpy statement of the same definition.

The case is pixel_cases.make's (40 000 lines, 2500-2560 cm-1 at 0.01, 6001 bins = 24 blocks of the kernel, the last one
ragged; 60 layers; both geometries).  The betas and what each is there for:

    1.037e-4    h = 25 -> 26    the half-width changes inside the grid
    1.3037e-3   h = 325 -> 333  a halo wider than a block; windows that reach the clip at both ends of the grid
    3.95e-6     h = 0 -> 1      the copy branch and the first window of three bins in one launch
    2e-6        h = 0           the identity

Every test first asserts that no d_i / wn_d comes within 1e-9 of an integer: a disagreement of one bin about h_i cannot
then be taken for rounding.

Tolerance, per bin, derived and not tuned: broaden.bound, tol_i = A_i (2 h_i + 17) 2^-52 + E_i against
broaden.reference (long-double weights, math.fsum) of the spectrum the same call returned.  A double walk in the
kernel's order stays within 0.06 of it on the CPU (tests/broaden_check.cpp; 0.6 at h = 1, where the one weight sits on
the profile's edge).  Where h_i = 0 the output must be the input's bits."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import pixel_cases as pc
import xcor_checks as xc
from cases import GOLDEN
from transit_amd import _abi, broaden, pixels, xcor
from transit_amd.engine import Batch, Engine, EngineError
from transit_amd.host import Problem

pytestmark = pytest.mark.gpu

SHIFTS = pc.SHIFTS
BETAS = {"h25-26": 1.037e-4, "h325-333": 1.3037e-3, "h0-1": 3.95e-6, "h0": 2e-6}
HALVES = {"h25-26": (25, 26), "h325-333": (325, 333), "h0-1": (0, 1), "h0": (0, 0)}
LIMBS = (0.0, 0.6, 1.0)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the problem of each geometry, made once for the module; and the references of the spectra seen so far (the hinted
    runs repeat the first run's bits: one reference serves them)"""
    made, refs = {}, {}

    def get(solution, **kw):
        key = (solution,) + tuple(sorted(kw.items()))
        if key not in made:
            made[key] = pc.make(tmp_path_factory.mktemp("broaden"), solution, **kw)
        return made[key]

    def reference(P, spec, b):
        key = (spec.tobytes(), b.beta, b.limb)
        if key not in refs:
            wn_i, wn_d, _, _ = pc.grid(P)
            ref = broaden.reference(spec, wn_i, wn_d, b)
            refs[key] = (ref, broaden.bound(spec, wn_i, wn_d, b, ref=ref))
        return refs[key]

    get.reference = reference
    return get


def margin(P, beta):
    """the smallest distance of a d_i / wn_d from an integer, and the half-widths"""
    wn_i, wn_d, n, _ = pc.grid(P)
    h, d = broaden._halves(wn_i, wn_d, n, beta)
    q = d / wn_d
    return float(np.min(np.abs(q - np.round(q)))), h


def check_broadened(case, P, b, got, spec, what=""):
    m, h = margin(P, b.beta)
    if not h.any():
        assert np.array_equal(got, spec), what
        return 0.0
    ref, tol = case.reference(P, spec, b)
    assert np.array_equal(got[h == 0], spec[h == 0]), what
    ratio = np.abs(got - ref)[h > 0] / tol[h > 0]
    worst = float(ratio.max())
    print("%s: largest |B - ref| / tol %.4f, largest relative error %.3e" % (what, worst, float(np.max(np.abs(got - ref) / np.abs(ref)))))
    assert worst <= 1.0, (what, worst)
    return worst


@pytest.mark.parametrize("limb", LIMBS)
@pytest.mark.parametrize("name", list(BETAS))
@pytest.mark.parametrize("solution", ["eclipse", "transit"])
def test_broadened_runs_keep_the_spectrum_and_match_the_definition(case, solution, name, limb):
    P = case(solution)
    assert P.nwn == 6001
    b = broaden.Rotation.from_beta(BETAS[name], limb)
    m, h = margin(P, b.beta)
    assert m >= 1e-9 and (h[0], h[-1]) == HALVES[name] and np.all(np.diff(h) >= 0), (m, h[0], h[-1])
    plain, E = Engine(P.static), Engine(P.static)
    E.set_broadening(b)
    deep, keep = pc.thinner(P, 1e-3)
    for k, atm in enumerate((P.atm, P.atm, deep, P.atm)):      # fresh, hinted, resuming deeper, hinted again
        ref = plain.run(atm, P.opts)["spectrum"]
        got, spec = E.run_broadened(atm, P.opts, spectrum=True)
        assert np.array_equal(spec, ref), k
        check_broadened(case, P, b, got, spec, "%s %s limb %g run %d" % (solution, name, limb, k))
        if h.any():
            assert not np.array_equal(got, spec)
    plain.close(); E.close()


@pytest.mark.parametrize("solution", ["eclipse", "transit"])
def test_pixels_moments_and_filter_sample_the_broadened_spectrum(case, solution):
    P = case(solution)
    wn_i, wn_d, n, _ = pc.grid(P)
    b = broaden.Rotation.from_beta(BETAS["h25-26"], 0.6)
    assert margin(P, b.beta)[0] >= 1e-9
    px = pc.joined(pc.set_a(P), pc.set_b(P))
    tol = pc.tolerance(px, SHIFTS)
    E, U = Engine(P.static), Engine(P.static)
    E.set_pixels(px); U.set_pixels(px)
    E.set_broadening(b)
    deep, keep = pc.thinner(P, 1e-3)
    for k, atm in enumerate((P.atm, deep)):
        B, spec = E.run_broadened(atm, P.opts, spectrum=True)
        pairs, spec2 = E.run_pixels(atm, P.opts, SHIFTS, spectrum=True)
        assert np.array_equal(spec2, spec)                # the plain spectrum, never the broadened one
        pc.check_close(pairs, pixels.reference(B, wn_i, wn_d, n, px, SHIFTS), tol, "%s run %d pairs vs reference over B" % (solution, k))
        plain_pairs = U.run_pixels(atm, P.opts, SHIFTS)
        moved = float(np.max(np.abs(pixels.value(pairs) - pixels.value(plain_pairs)) / np.abs(pixels.value(plain_pairs))))
        print("%s run %d: broadening moves the pixel values by up to %.3e (tolerance %.3e)" % (solution, k, moved, tol))
        assert moved > 1e4 * tol
        assert np.array_equal(pairs[..., 1], plain_pairs[..., 1])      # the weights' sums know nothing of the spectrum
    # moments and filtered moments on the same handle: over those pairs, at those files' own bounds
    pairs = E.run_pixels(P.atm, P.opts, SHIFTS)
    ob = xc.observed(len(px), float(np.mean(spec)))
    E.set_observed(ob)
    mom = E.run_moments(P.atm, P.opts, SHIFTS)
    xc.check_moments(mom, pairs, ob, "%s moments over broadened pairs" % solution)
    F = xcor.svd_filter(ob.data, ob.seg_first, 3)
    E.set_filter(F)
    fmom, val = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    xc.check_values(val, pairs, ob, F, "%s filtered values over broadened pairs" % solution)
    xc.check_filtered_moments(fmom, val, ob, "%s filtered moments" % solution)
    assert not np.isnan(val).any()
    U.set_observed(ob)
    assert not np.array_equal(U.run_moments(P.atm, P.opts, SHIFTS), mom)
    E.close(); U.close()


def test_bits_do_not_depend_on_the_rest_of_the_call(case):
    P = case("eclipse")
    b = broaden.Rotation.from_beta(BETAS["h325-333"], 0.6)
    assert margin(P, b.beta)[0] >= 1e-9
    px = pc.joined(pc.set_a(P), pc.set_b(P))
    bs = pc.band_set(P)
    E, U, fresh = Engine(P.static), Engine(P.static), Engine(P.static)
    for X in (E, U, fresh):
        X.set_pixels(px)
        X.set_bands(bs)
    E.set_broadening(b); fresh.set_broadening(b)
    first = E.run_broadened(P.atm, P.opts)
    for _ in range(2):
        assert np.array_equal(E.run_broadened(P.atm, P.opts), first)
    assert np.array_equal(E.run_broadened(P.atm, P.opts, spectrum=True)[0], first)
    # run_broadened, then run_pixels on the same handle: the pairs of a handle that never made a broadened run
    want = fresh.run_pixels(P.atm, P.opts, SHIFTS)
    assert np.array_equal(E.run_pixels(P.atm, P.opts, SHIFTS), want)
    assert np.array_equal(E.run_broadened(P.atm, P.opts), first)
    assert np.array_equal(E.run_pixels(P.atm, P.opts, SHIFTS, spectrum=True)[0], want)
    # the runs that stay as they are, whatever is installed
    plain = U.run_pixels(P.atm, P.opts, SHIFTS)
    assert not np.array_equal(want, plain)
    deep, keep = pc.thinner(P, 1e-3)
    for atm in (P.atm, deep):
        assert np.array_equal(E.run(atm, P.opts)["spectrum"], U.run(atm, P.opts)["spectrum"])
        se, sp_e = E.run_bands(atm, P.opts, spectrum=True)
        su, sp_u = U.run_bands(atm, P.opts, spectrum=True)
        assert np.array_equal(se, su) and np.array_equal(sp_e, sp_u)
        ce, cu = E.run_contrib(atm, P.opts), U.run_contrib(atm, P.opts)
        assert np.array_equal(ce[0], cu[0]) and np.array_equal(ce[1], cu[1])
    # set_pixels does not drop the broadening; clearing it gives the parent's pair bits again
    E.set_pixels(px)
    assert np.array_equal(E.run_pixels(P.atm, P.opts, SHIFTS), want)
    E.set_broadening(None)
    assert np.array_equal(E.run_pixels(P.atm, P.opts, SHIFTS), plain)
    assert margin(P, BETAS["h0"])[0] >= 1e-9
    E.set_broadening(broaden.Rotation.from_beta(BETAS["h0"], 0.6))      # h = 0 everywhere: a copy, the same pairs
    assert np.array_equal(E.run_pixels(P.atm, P.opts, SHIFTS), plain)
    E.close(); U.close(); fresh.close()


def test_batch_outputs_are_the_single_handle_outputs(case):
    P = case("eclipse", nlines=30_000, seed=33)
    px = pc.joined(pc.set_a(P), pc.set_b(P))
    K = 5
    atms, keep = pc.atmospheres(P, K)
    bl = [broaden.Rotation.from_beta(beta, limb) for beta, limb in
          ((1.037e-4, 0.6), (1.3037e-3, 0.0), (3.95e-6, 1.0), (2e-6, 0.3), (5.2037e-4, 0.85))]
    for b in bl:
        assert margin(P, b.beta)[0] >= 1e-9
    shifts = np.stack([np.roll(SHIFTS, j)[:5] * (1.0 + 1e-6 * j) for j in range(K)])
    ob = xc.observed(len(px), 1.0, nexp=5)
    F = xcor.svd_filter(ob.data, ob.seg_first, 2)
    one = Engine(P.static)
    one.set_pixels(px); one.set_observed(ob); one.set_filter(F)
    own, same = {}, {}                                   # every atmosphere under its own broadening; all under the first
    for dest, pick in ((own, lambda j: bl[j]), (same, lambda j: bl[0])):
        for what in ("broadened", "pixels", "moments", "filtered"):
            dest[what] = []
        for j in range(K):
            one.set_broadening(pick(j))
            dest["broadened"].append(one.run_broadened(atms[j], P.opts))
            dest["pixels"].append(one.run_pixels(atms[j], P.opts, shifts[j]))
            dest["moments"].append(one.run_moments(atms[j], P.opts, shifts[j]))
            dest["filtered"].append(one.run_filtered_moments(atms[j], P.opts, shifts[j]))
    one.set_broadening(None)
    bare = [one.run_pixels(atms[j], P.opts, shifts[j]) for j in range(K)]
    plain = [one.run(atms[j], P.opts)["spectrum"] for j in range(K)]
    one.close()
    assert len({x.tobytes() for x in own["broadened"]}) == K
    B = Batch(P.static, ways=3)
    B.set_pixels(px); B.set_observed(ob); B.set_filter(F)
    with pytest.raises(EngineError) as ei:              # nothing installed
        B.run_broadened(atms, P.opts)
    assert ei.value.code == -1
    assert np.array_equal(B.run_pixels(atms, P.opts, shifts), np.stack(bare))
    for install, want in ((bl, own), (bl[0], same), ([bl[0]], same)):
        B.set_broadening(install)
        for rep in range(2):
            assert np.array_equal(B.run_broadened(atms, P.opts), np.stack(want["broadened"])), rep
            assert np.array_equal(B.run_pixels(atms, P.opts, shifts), np.stack(want["pixels"])), rep
        assert np.array_equal(B.run_moments(atms, P.opts, shifts), np.stack(want["moments"]))
        assert np.array_equal(B.run_filtered_moments(atms, P.opts, shifts), np.stack(want["filtered"]))
        assert np.array_equal(B.run(atms, P.opts), np.stack(plain))      # trx_run_batch ignores it
    # three broadenings for five atmospheres: every such run is refused, and nothing changes
    B.set_broadening(bl[:3])
    for run in (lambda: B.run_broadened(atms, P.opts), lambda: B.run_pixels(atms, P.opts, shifts),
                lambda: B.run_moments(atms, P.opts, shifts), lambda: B.run_filtered_moments(atms, P.opts, shifts)):
        with pytest.raises(EngineError) as ei:
            run()
        assert ei.value.code == -1 and "3 broadenings" in str(ei.value)
    assert np.array_equal(B.run_broadened(atms[:3], P.opts), np.stack(own["broadened"][:3]))
    assert np.array_equal(B.run(atms, P.opts), np.stack(plain))
    # all entries are checked before any is kept
    with pytest.raises(EngineError) as ei:
        B.set_broadening(bl[:2] + [broaden.Rotation.from_beta(1e-4, 1.5)])
    assert ei.value.code == -1 and "entry 2" in str(ei.value) and "limb" in str(ei.value)
    assert np.array_equal(B.run_broadened(atms[:3], P.opts), np.stack(own["broadened"][:3]))
    B.set_broadening(None)                              # cleared: the pixels see the plain spectrum again
    assert np.array_equal(B.run_pixels(atms, P.opts, shifts), np.stack(bare))
    with pytest.raises(EngineError):
        B.run_broadened(atms, P.opts)
    B.close()


def test_opacity_grid_handle(tmp_path, case):
    d = tmp_path / "og"
    shutil.copytree(os.path.join(GOLDEN, "opacity_grid"), d)
    P = Problem.from_cfg(os.path.join(str(d), "case.cfg"))
    builder = Engine(P.static)
    builder.build_opacity_grid(P)
    builder.close()
    assert P.static.ogrid
    wn_i, wn_d, n, wn = pc.grid(P)
    b = broaden.Rotation.from_beta(5.37 * wn_d / float(wn[-1]), 0.6)
    m, h = margin(P, b.beta)
    assert m >= 1e-9 and h[-1] == 5 and 2 * h[-1] < n < 256, (m, h[0], h[-1], n)      # one ragged block, clipped at both ends
    plain, E = Engine(P.static), Engine(P.static)
    E.set_broadening(b)
    for k in range(2):
        ref = plain.run(P.atm, P.opts)["spectrum"]
        got, spec = E.run_broadened(P.atm, P.opts, spectrum=True)
        assert np.array_equal(spec, ref)
        check_broadened(case, P, b, got, spec, "opacity grid run %d" % k)
        assert np.array_equal(E.run(P.atm, P.opts)["spectrum"], ref)
    plain.close(); E.close()


def test_refusals_and_lifetime(case):
    P = case("eclipse", nlines=10_000)
    wn_i, wn_d, n, wn = pc.grid(P)
    E = Engine(P.static)
    lib = E._lib
    with pytest.raises(EngineError) as ei:              # nothing installed
        E.run_broadened(P.atm, P.opts)
    assert ei.value.code == -1 and "no broadening" in str(ei.value)
    good = broaden.Rotation.from_beta(BETAS["h25-26"], 0.6)
    assert margin(P, good.beta)[0] >= 1e-9
    E.set_broadening(good)
    before = E.run_broadened(P.atm, P.opts)
    bad = {"beta nan": (np.nan, 0.6), "beta inf": (np.inf, 0.6), "beta 0": (0.0, 0.6), "beta < 0": (-1e-4, 0.6),
           "limb nan": (1e-4, np.nan), "limb inf": (1e-4, np.inf), "limb < 0": (1e-4, -0.01), "limb > 1": (1e-4, 1.01)}
    for what, (beta, limb) in bad.items():
        with pytest.raises(EngineError) as ei:
            E.set_broadening(broaden.Rotation.from_beta(beta, limb))
        assert ei.value.code == -1 and what.split()[0] in str(ei.value), what
        assert np.array_equal(E.run_broadened(P.atm, P.opts), before), what      # the old one is still in force
    c = _abi.TrxBroadening(7, 0, 1e-4, 0.6)
    assert lib.trx_set_broadening(E._h, C.byref(c)) == -1 and b"unknown kind 7" in lib.trx_last_error(E._h)
    # the cap: h at the grid's last bin 2049 is refused and named, 2048 is accepted and runs
    over, at = broaden.Rotation.from_beta(8.0043e-3, 0.6), broaden.Rotation.from_beta(8.0002e-3, 0.6)
    assert margin(P, over.beta)[1][-1] == 2049 and margin(P, at.beta)[1][-1] == 2048 == broaden.MAX_HALF
    assert margin(P, over.beta)[0] >= 1e-9 and margin(P, at.beta)[0] >= 1e-9
    with pytest.raises(EngineError) as ei:
        E.set_broadening(over)
    assert ei.value.code == -1 and "2049" in str(ei.value)
    assert np.array_equal(E.run_broadened(P.atm, P.opts), before)
    E.set_broadening(at)
    wide, spec = E.run_broadened(P.atm, P.opts, spectrum=True)
    bins = [0, 1, 255, 256, 2047, 2048, 3000, n - 2049, n - 2048, n - 1]
    ref = broaden.reference(spec, wn_i, wn_d, at, bins=bins)
    tol = broaden.bound(spec, wn_i, wn_d, at, bins=bins, ref=ref)
    print("h = 2048: largest |B - ref| / tol %.4f over %d bins" % (float(np.max(np.abs(wide[bins] - ref) / tol)), len(bins)))
    assert np.all(np.abs(wide[bins] - ref) <= tol)
    # the run's own refusal; a cleared broadening is refused again
    E.set_broadening(good)
    dp = _abi.c_double_p
    out = np.zeros(n)
    assert lib.trx_run_broadened(E._h, C.byref(P.atm), C.byref(P.opts), None, None, None) == -1
    assert lib.trx_run_broadened(E._h, C.byref(P.atm), C.byref(P.opts), None, out.ctypes.data_as(dp), None) == 0
    assert np.array_equal(out, before)
    none = _abi.TrxBroadening(_abi.BROADEN_NONE, 0, np.nan, np.nan)      # kind NONE clears, whatever else it holds
    assert lib.trx_set_broadening(E._h, C.byref(none)) == 0
    with pytest.raises(EngineError):
        E.run_broadened(P.atm, P.opts)
    E.set_broadening(good)
    E.set_pixels(pixels.Pixels([2510.0, 2520.0], [0.2, 0.3], 4.0))       # set_pixels does not drop it
    assert np.array_equal(E.run_broadened(P.atm, P.opts), before)
    E.set_pixels(None)
    assert np.array_equal(E.run_broadened(P.atm, P.opts), before)
    E.set_broadening(None)
    with pytest.raises(EngineError):
        E.run_broadened(P.atm, P.opts)
    E.close()
    # a handle whose shard is not the whole grid: the window needs neighbours across its edge
    try:
        P.set_shard(1500, n)
        S = Engine(P.static)
        with pytest.raises(EngineError) as ei:
            S.set_broadening(good)
        assert ei.value.code == -6 and "shard" in str(ei.value)
        S.set_broadening(None)                           # clearing is always allowed
        with pytest.raises(EngineError):
            S.run_broadened(P.atm, P.opts)
        S.close()
    finally:
        P.set_shard(0, n)


@pytest.mark.parametrize("field,value", [("wn_i", 0.0), ("wn_i", -2500.0), ("wn_d", 0.0), ("wn_d", -0.01)])
def test_a_grid_that_does_not_start_or_step_above_zero_is_refused(case, field, value):
    """trx_create does not look at wn_i or wn_d and, without lines, nothing it makes depends on them: such a handle exists,
    and the half-widths mean nothing on it.  No run is made on it."""
    P = case("eclipse", nlines=10_000)
    good = broaden.Rotation.from_beta(BETAS["h25-26"], 0.6)
    assert margin(P, good.beta)[0] >= 1e-9
    st = _abi.TrxStatic.from_buffer_copy(P.static)
    st.nlines = 0
    setattr(st, field, value)
    E = Engine(st)
    with pytest.raises(EngineError) as ei:
        E.set_broadening(good)
    assert ei.value.code == -1 and "wn_i > 0 and wn_d > 0" in str(ei.value)
    # the argument's own faults are named first, the grid's ahead of the half-width (which a wn_d of 0 would make infinite)
    with pytest.raises(EngineError) as ei:
        E.set_broadening(broaden.Rotation.from_beta(good.beta, 1.5))
    assert ei.value.code == -1 and "limb" in str(ei.value)
    with pytest.raises(EngineError) as ei:              # nothing was kept
        E.run_broadened(P.atm, P.opts)
    assert ei.value.code == -1 and "no broadening" in str(ei.value)
    E.set_broadening(None)                              # clearing is always allowed
    E.close()
