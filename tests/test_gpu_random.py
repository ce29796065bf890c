"""Seeded random problems: the HIP path against the CPU oracle over corners of the parameter
space no hand-written case sits on (tests/random_cases.py: oversampling 1..2160, 3..200 layers
on both sides of the walk step and the ray tail's limit, 0..5000 lines in bands of 2..40 cm-1
over 1-3 databases of 2..256 isotopes, thresholds from 1e-50 to 1e-3, both geometries, 1..16
angles, 0..2 CIA tables, clouds and scattering).  On one handle: the first run, hinted runs,
the atmosphere made thinner and denser under the remembered depth (the pass resumed, a shorter
plan), each against the oracle for that atmosphere; then a batch of the atmospheres, bit for bit
the single handle's spectra.  Shards of the spectrum must be slices of the full run, bit for bit.
A second sweep draws one of the kernels' A/B switches per seed and requires the default form's bits.  The last test asserts
that the sweep reached the edges it is there for (test_random_reference.py pins the oracle to
the compiled reference on the same seeds)."""
import ctypes as C
import os

import numpy as np
import pytest

import random_cases
from cases import rel_err
from tolerances import KEYS, assert_same, check_against_oracle, oracle
from transit_amd import _abi, engine, synth
from transit_amd.engine import Batch, Engine, EngineError
from transit_amd.host import Problem

pytestmark = pytest.mark.gpu

NCASES = int(os.environ.get("TRX_RANDOM_CASES", "48"))
NSWITCH = max(1, NCASES // 2)
SCALES = (0.03, 40.0)          # density factors: the hint too shallow (resumed), then too deep (shorter plan)
# the A/B switches of the kernel forms (values: the alternatives to the default form)
SWITCHES = [("TRX_LANES_WALK", ("0", "2")), ("TRX_NO_PACKED_WALK", ("1",)), ("TRX_PACKED_MAX_LAYERS", ("1", "3", "32")),
            ("TRX_NO_ROW_STAGING", ("1",)), ("TRX_NO_BINREC", ("1",)), ("TRX_TWO_QUEUES", ("0",)), ("TRX_RAY_TAIL", ("0",)),
            ("TRX_XCD_MAP", ("0", "3")), ("TRX_CIA_SUMS", ("0",))]
# what the sweeps met, per seed (test_random_sweep_reached_its_edges)
SEEN = {"cases": set(), "switch_cases": set(), "tail": set(), "deep_plan": set(), "isotopes_over_64": set(),
        "angles_over_8": set(), "switches": []}


def make_problem(tmp_path, seed):
    kw = random_cases.random_case(seed)
    d = str(tmp_path / "r")
    synth.make_case(d, **kw)
    return Problem.from_cfg(os.path.join(d, "case.cfg")), random_cases.summary(kw)


def scaled_atmosphere(P, dens, f):
    """A copy of the problem's atmosphere with its densities times f (the array is returned with it)."""
    d = np.ascontiguousarray(dens * f)
    a = _abi.TrxAtm()
    C.memmove(C.byref(a), C.byref(P.atm), C.sizeof(_abi.TrxAtm))
    a.density = d.ctypes.data_as(_abi.c_double_p)
    return a, d


def note_coverage(seed, P, hip, msgs):
    if any("ray tail over" in m for m in msgs):
        SEEN["tail"].add(seed)
    if hip.stats()["walk_steps"] >= 3:
        SEEN["deep_plan"].add(seed)
    if P.static.niso > 64:
        SEEN["isotopes_over_64"].add(seed)
    if P.opts.solution == 0 and P.opts.nangles > 8:
        SEEN["angles_over_8"].add(seed)


@pytest.mark.parametrize("seed", range(NCASES))
def test_random_problem_against_oracle(tmp_path, seed):
    P, kw = make_problem(tmp_path, seed)
    dens = np.ctypeslib.as_array(P.atm.density, shape=(P.static.nmol * P.nlayer,))
    base = dens.copy()
    msgs = []
    engine.set_log(lambda lvl, m: msgs.append(m), 5)
    hip = Engine(P.static)
    spectra = {}
    try:
        ref = oracle(P)
        for rep in range(3):                        # first run, then hinted runs
            got = check_against_oracle(P, hip, ref, (kw, rep))
            note_coverage(seed, P, hip, msgs)
        spectra[1.0] = None if got is None else got["spectrum"]
        for sc in SCALES:                           # the atmosphere moves under the remembered depth
            dens[:] = base * sc
            got = check_against_oracle(P, hip, oracle(P), (kw, sc))
            note_coverage(seed, P, hip, msgs)
            spectra[sc] = None if got is None else got["spectrum"]
    finally:
        dens[:] = base
        engine.set_log(None)
        hip.close()
    SEEN["cases"].add(seed)
    if spectra[1.0] is None:
        return
    # a batch of the three atmospheres: each spectrum the single handle's, bit for bit
    if all(spectra[sc] is not None for sc in SCALES):
        keep = [scaled_atmosphere(P, base, f) for f in (1.0,) + SCALES]
        B = Batch(P.static, ways=3)
        try:
            got = B.run([a for a, _ in keep], P.opts)
        finally:
            B.close()
        for j, f in enumerate((1.0,) + SCALES):
            assert np.array_equal(got[j], spectra[f]), (kw, f)


@pytest.mark.parametrize("seed", range(NCASES))
def test_random_shards_are_slices_of_the_full_run(tmp_path, seed):
    """A one-ray shard and a random range (most often with a ragged last block of rays): the full run's
    spectrum slice on the shard handle's first and hinted runs -- bit for bit where every layer walks
    its lines; to 1e-12 where some layer takes the two-kernel form."""
    P, kw = make_problem(tmp_path, seed)
    msgs = []
    engine.set_log(lambda lvl, m: msgs.append(m), 5)
    hip = Engine(P.static)
    full = None
    try:
        hip.run(P.atm, P.opts)
        full = hip.run(P.atm, P.opts)["spectrum"]
    except EngineError as e:                        # a refused case: every shard is refused the same way
        refused = e
    finally:
        engine.set_log(None)
        hip.close()
    frames = [m.split(":")[-1].split() for m in msgs if "walk frame (bins) per layer" in m]
    two_kernel = not frames or "0" in frames[-1]
    rng = np.random.default_rng(7000 + seed)
    nwn = P.nwn
    k = int(rng.integers(0, nwn))
    lo = int(rng.integers(0, nwn))
    hi = lo + 1 + int(rng.integers(0, nwn - lo))
    try:
        for lo_, hi_ in [(k, k + 1), (lo, hi)]:
            P.set_shard(lo_, hi_)
            sh = Engine(P.static)
            try:
                for rep in range(2):
                    if full is None:
                        with pytest.raises(EngineError) as ei:
                            sh.run(P.atm, P.opts)
                        assert ei.value.code == refused.code, (kw, lo_, hi_, rep)
                        continue
                    got = sh.run(P.atm, P.opts)["spectrum"]
                    note = (kw, lo_, hi_, rep, rel_err(got, full[lo_:hi_]))
                    if two_kernel:
                        assert rel_err(got, full[lo_:hi_]) < 1e-12 and np.array_equal(got == 0, full[lo_:hi_] == 0), note
                    else:
                        assert np.array_equal(got, full[lo_:hi_]), note
            finally:
                sh.close()
    finally:
        P.set_shard(0, nwn)


@pytest.mark.parametrize("seed", range(NSWITCH))
def test_random_problem_under_a_form_switch(tmp_path, seed):
    """One A/B switch per seed (set around Engine() only, as the form tests do): the switched handle
    gives the default handle's bits through the same runs -- first, hinted, thinner, denser, back."""
    P, kw = make_problem(tmp_path, seed)
    name, values = SWITCHES[seed % len(SWITCHES)]
    value = str(np.random.default_rng(9000 + seed).choice(values))
    SEEN["switches"].append("%s=%s" % (name, value))
    os.environ[name] = value
    try:
        b = Engine(P.static)
    finally:
        os.environ.pop(name, None)
    a = Engine(P.static)
    dens = np.ctypeslib.as_array(P.atm.density, shape=(P.static.nmol * P.nlayer,))
    base = dens.copy()
    try:
        for k, sc in enumerate([1.0, 1.0, 1.0, SCALES[0], SCALES[1], 1.0]):
            dens[:] = base * sc
            note = (kw, name, value, k, sc)
            dbg = KEYS if k != 2 else None          # (one production run without debug copies)
            try:
                ra = a.run(P.atm, P.opts, debug=dbg) if dbg else a.run(P.atm, P.opts)
            except EngineError as e:
                with pytest.raises(EngineError) as ei:
                    b.run(P.atm, P.opts, debug=dbg) if dbg else b.run(P.atm, P.opts)
                assert ei.value.code == e.code, note
                continue
            rb = b.run(P.atm, P.opts, debug=dbg) if dbg else b.run(P.atm, P.opts)
            assert_same(ra, rb, note)
            assert a.stats()["layers_swept"] == b.stats()["layers_swept"], note
    finally:
        dens[:] = base
        a.close(); b.close()
    SEEN["switch_cases"].add(seed)


def test_random_sweep_reached_its_edges():
    """Coverage is asserted, not assumed: over the sweep, k_ray_tail ran for at least 5 seeds, plans of 3 or
    more walk steps for at least 3, more than 64 isotopes for at least 3, more than 8 angles for at least one."""
    if len(SEEN["cases"]) < NCASES or len(SEEN["switch_cases"]) < NSWITCH:
        pytest.skip("the random sweeps did not run in full in this session")
    counts = {k: len(v) for k, v in SEEN.items() if k not in ("cases", "switch_cases", "switches")}
    print("random sweep: %d + %d seeds, %s, switches %s" % (NCASES, NSWITCH, counts, " ".join(SEEN["switches"])))
    assert counts["tail"] >= 5, counts
    assert counts["deep_plan"] >= 3, counts
    assert counts["isotopes_over_64"] >= 3, counts
    assert counts["angles_over_8"] >= 1, counts
