"""Seeded opacity-grid problems (random_cases.random_grid_case): the per-molecule sweep
(trx_sweep_permol, calcopacity() on the GPU) and grid-mode runs (k_grid_extinction) against the CPU
oracle, at state counts around the sweep's 64-state steps (short last steps in the packed and lanes
forms, sweeps that mix walk and two-kernel steps), 1-3 molecule slots of 2..256 isotopes, isotopes and
whole slots without lines, thresholds from 1e-50 to 1e-3 and grids from 70 to 3000 K.

Per seed: the sweep in the host's slot layout and in one other legal layout against the oracle; a
state's row against the same state swept in other company (reversed, a subset, alone) and on shards;
the sweep under one kernel-form switch; a handle that sweeps between spectra; the grid-mode spectrum
and extinction for the atmosphere as written, moved and on the grid's nodes and edges.  The last test
asserts that the seeds reached the edges they are there for (test_random_grid_reference.py pins the
oracle to the compiled reference on the same seeds).

Where a row must keep its bits: a state's sums are in line order whatever its company, as long as it
walks its lines (the walk's form follows the state, walk_frame_bins); the two-kernel form sums a bin
in an order that depends on the step, so there 1e-12 and the same zero pattern."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
import random_cases
from cases import rel_err
from tolerances import check_against_oracle, oracle
from transit_amd import _abi, engine, synth
from transit_amd.engine import Batch, Engine, EngineError
from transit_amd.host import Problem

pytestmark = pytest.mark.gpu

NCASES = int(os.environ.get("TRX_RANDOM_GRID_CASES", "48"))
# the A/B switches of the kernel forms (values: the alternatives to the default form)
SWITCHES = [("TRX_LANES_WALK", ("0", "2")), ("TRX_LANES_PARTS", ("2", "3")), ("TRX_NO_PACKED_WALK", ("1",)),
            ("TRX_PACKED_MAX_LAYERS", ("1", "3", "32")), ("TRX_NO_ROW_STAGING", ("1",)), ("TRX_NO_ROWS32", ("1",)),
            ("TRX_NO_ROW_COPY", ("1",)), ("TRX_NO_BINREC", ("1",)), ("TRX_XCD_MAP", ("0", "3"))]
# what the sweeps met, per seed (test_random_grid_sweep_reached_its_edges)
SEEN = {"sweep_cases": set(), "grid_cases": set(), "short_last_step": set(), "mixed": set(), "lanes": set(),
        "packed": set(), "slots_over_2": set(), "isotopes_over_64": set(), "empty_slot": set(), "nv_over_2000": set(),
        "switches": []}
FULL = {"walk": 64, "lanes": 64, "packed": 64, "two-kernel": 12}
_LOG = []


def _log(level, msg):
    _LOG.append(msg)


def make_problem(tmp_path, seed):
    kw = random_cases.random_grid_case(seed)
    d = str(tmp_path / "g")
    synth.make_case(d, **kw)
    return Problem.from_cfg(os.path.join(d, "case.cfg")), kw, random_cases.summary(kw)


def states(P):
    """The grid's (layer x temperature) states as numpy arrays (Problem.grid_request)."""
    nv, t, d, z, nslot, sl = P.grid_request()
    nm, ni = P.static.nmol, P.static.niso
    arr = lambda p, n: np.ctypeslib.as_array(p, shape=(n,)).copy()
    return dict(nv=nv, temp=arr(t, nv), dens=arr(d, nm * nv).reshape(nm, nv), z=arr(z, ni * nv).reshape(ni, nv),
                nslot=nslot, slots=arr(sl, ni).astype(np.int32))


def sweep(eng, S, idx=None, ethresh=None, nslot=None, slots=None):
    """o[state][slot][bin] of the states idx (all: None) and the step plan the HIP sweep logged
    [(form, states, frame bins)] (the oracle logs none)."""
    idx = np.arange(S["nv"]) if idx is None else np.asarray(idx)
    t = np.ascontiguousarray(S["temp"][idx])
    d = np.ascontiguousarray(S["dens"][:, idx]); z = np.ascontiguousarray(S["z"][:, idx])
    sl = np.ascontiguousarray(S["slots"] if slots is None else slots, dtype=np.int32)
    del _LOG[:]
    out = eng.sweep_permol(len(idx), t.ctypes.data_as(_abi.c_double_p), d.ctypes.data_as(_abi.c_double_p),
                           z.ctypes.data_as(_abi.c_double_p), S["ethresh"] if ethresh is None else ethresh,
                           S["nslot"] if nslot is None else nslot, sl.ctypes.data_as(_abi.c_int32_p))
    steps = []
    for m in _LOG:
        if m.startswith("sweep step: "):
            f = dict(kv.strip().rsplit(" ", 1) for kv in m[len("sweep step: "):].split(","))
            steps.append((f["form"], int(f["states"]), int(f["frame bins"])))
    del _LOG[:]
    assert not steps or sum(s[1] for s in steps) == len(idx), steps
    return out, steps


def all_walk(*plans):
    return all(f != "two-kernel" for p in plans for f, _, _ in p)


def assert_rows(got, want, plans, note):
    """The company rule: bit for bit where every state of both sweeps walks its lines, else 1e-12 and the same zeros."""
    if all_walk(*plans):
        assert np.array_equal(got, want), (note, rel_err(got, want))
    else:
        assert np.array_equal(got == 0, want == 0), note
        assert rel_err(got, want) < 1e-12, (note, rel_err(got, want))


def other_layout(S, seed):
    """One more legal slot layout per seed, rotating: every isotope in one slot; more slots than used; one
    molecule split in two contiguous slots.  (nslot, iso_slot, name)"""
    slots, nslot = S["slots"], S["nslot"]
    kind = seed % 3
    if kind == 2:
        counts = np.bincount(slots, minlength=nslot)
        split = [s for s in range(nslot) if counts[s] >= 2]
        if split:
            s = split[seed % len(split)]
            first = int(np.flatnonzero(slots == s)[0])
            cut = first + 1 + (seed // 3) % (int(counts[s]) - 1)
            new = slots.copy()
            new[cut:] += 1
            return nslot + 1, new, "split slot %d at isotope %d" % (s, cut)
        kind = 0
    if kind == 1:
        return nslot + 2, slots.copy(), "two unused slots"
    return 1, np.zeros_like(slots), "one slot"


def empty_slots(kw, S):
    """Host slots none of whose isotopes has a line in the band (random_grid_case: whole databases)."""
    counts = [len(w) for db in kw["dbs"] for w in db.wl]
    has = np.zeros(S["nslot"], dtype=bool)
    for i, c in enumerate(counts):
        has[S["slots"][i]] |= c > 0
    return np.flatnonzero(~has)


def note_coverage(seed, P, S, kw, plan):
    forms = [f for f, _, _ in plan]
    if len(plan) >= 2 and plan[-1][1] < 17 and plan[-2][1] == FULL[plan[-2][0]]:
        SEEN["short_last_step"].add(seed)
    if "two-kernel" in forms and any(f != "two-kernel" for f in forms):
        SEEN["mixed"].add(seed)
    if "lanes" in forms:
        SEEN["lanes"].add(seed)
    if "packed" in forms:
        SEEN["packed"].add(seed)
    if S["nslot"] > 2:
        SEEN["slots_over_2"].add(seed)
    if P.static.niso > 64:
        SEEN["isotopes_over_64"].add(seed)
    if len(empty_slots(kw, S)):
        SEEN["empty_slot"].add(seed)
    if S["nv"] >= 2000:
        SEEN["nv_over_2000"].add(seed)


@pytest.fixture(autouse=True)
def _sweep_log():
    engine.set_log(_log, 5)
    yield
    engine.set_log(None)
    del _LOG[:]


@pytest.mark.parametrize("seed", range(NCASES))
def test_random_grid_sweep_against_oracle(tmp_path, seed):
    """The host's slot layout and one other against trxo_sweep_permol; then the same states in other company
    (reversed, a random subset, one at a time) and a repeat."""
    P, kw, note = make_problem(tmp_path, seed)
    S = states(P)
    S["ethresh"] = P.opts.ethresh
    hip, ora = Engine(P.static), ol.OracleEngine(P.static)
    try:
        full, plan = sweep(hip, S)
        layouts = [(S["nslot"], S["slots"], "host")] + [other_layout(S, seed)]
        for nslot, slots, name in layouts:
            a = full if name == "host" else sweep(hip, S, nslot=nslot, slots=slots)[0]
            b = sweep(ora, S, nslot=nslot, slots=slots)[0]
            n = (note, name, S["nv"], plan)
            assert a.shape == (S["nv"], nslot, P.nwn), n
            assert np.isfinite(a).all(), n
            assert np.array_equal(a == 0, b == 0), n
            assert rel_err(a, b) < 1e-10, (n, rel_err(a, b))
            if nslot > slots.max() + 1:
                assert not a[:, slots.max() + 1:].any(), n           # unused slots: exactly zero
        assert (full != 0).any(), note
        for s in empty_slots(kw, S):
            assert not full[:, s].any(), (note, "slot without lines", s)
        # a state's row does not depend on its company
        rng = np.random.default_rng(11000 + seed)
        rev, prev = sweep(hip, S, idx=np.arange(S["nv"])[::-1])
        assert_rows(rev[::-1], full, (plan, prev), (note, "reversed"))
        sub = rng.choice(S["nv"], size=int(rng.integers(1, S["nv"] + 1)), replace=False)
        got, psub = sweep(hip, S, idx=sub)
        assert_rows(got, full[sub], (plan, psub), (note, "subset", len(sub)))
        for v in rng.choice(S["nv"], size=min(3, S["nv"]), replace=False):
            got, pone = sweep(hip, S, idx=[v])
            assert_rows(got[0], full[v], (plan, pone), (note, "alone", int(v)))
        again, _ = sweep(hip, S)
        assert np.array_equal(again, full), note
    finally:
        hip.close(); ora.close()
    note_coverage(seed, P, S, kw, plan)
    SEEN["sweep_cases"].add(seed)


@pytest.mark.parametrize("seed", range(NCASES))
def test_random_grid_sweep_under_a_form_switch_and_on_shards(tmp_path, seed):
    """One A/B switch per seed (set around Engine() only): the default handle's bits.  A one-bin shard and a
    random [lo, hi): the full sweep's slice, under the company rule."""
    P, kw, note = make_problem(tmp_path, seed)
    S = states(P)
    S["ethresh"] = P.opts.ethresh
    name, values = SWITCHES[seed % len(SWITCHES)]
    value = str(np.random.default_rng(9500 + seed).choice(values))
    SEEN["switches"].append("%s=%s" % (name, value))
    os.environ[name] = value
    try:
        b = Engine(P.static)
    finally:
        os.environ.pop(name, None)
    a = Engine(P.static)
    try:
        full, plan = sweep(a, S)
        got, _ = sweep(b, S)
        assert np.array_equal(got, full), (note, name, value, rel_err(got, full))
    finally:
        a.close(); b.close()
    rng = np.random.default_rng(12000 + seed)
    nwn = P.nwn
    k = int(rng.integers(0, nwn))
    lo = int(rng.integers(0, nwn))
    hi = lo + 1 + int(rng.integers(0, nwn - lo))
    try:
        for lo_, hi_ in [(k, k + 1), (lo, hi)]:
            P.set_shard(lo_, hi_)
            sh = Engine(P.static)
            try:
                got, psh = sweep(sh, S)
            finally:
                sh.close()
            assert got.shape == (S["nv"], S["nslot"], hi_ - lo_), note
            assert_rows(got, full[:, :, lo_:hi_], (plan, psh), (note, "shard", lo_, hi_))
    finally:
        P.set_shard(0, nwn)


@pytest.mark.parametrize("seed", range(NCASES))
def test_random_grid_sweeps_between_spectra(tmp_path, seed):
    """trx_run, a hinted trx_run, a sweep of every state, a smaller sweep of other states (other temperatures
    and pressures at each state index: stale per-slot maxima would move the cut), then trx_run: the smaller
    sweep gives a fresh handle's rows, the last spectrum the hinted run's bits and depth."""
    P, kw, note = make_problem(tmp_path, seed)
    S = states(P)
    S["ethresh"] = 1e-3                          # (a threshold that cuts lines)
    small = np.arange(S["nv"])[::-1][:max(1, (S["nv"] + 1) // 2)]
    hip = Engine(P.static)
    try:
        try:
            hip.run(P.atm, P.opts)
            hinted = hip.run(P.atm, P.opts)["spectrum"]
            depth = hip.stats()["layers_swept"]
        except EngineError as e:
            hinted, refused = None, e
        big, _ = sweep(hip, S)
        got, _ = sweep(hip, S, idx=small)
        if hinted is None:
            with pytest.raises(EngineError) as ei:
                hip.run(P.atm, P.opts)
            assert ei.value.code == refused.code, note
        else:
            last = hip.run(P.atm, P.opts)["spectrum"]
            assert np.array_equal(last, hinted), (note, rel_err(last, hinted))
            assert hip.stats()["layers_swept"] == depth, note
    finally:
        hip.close()
    fresh = Engine(P.static)
    try:
        want, _ = sweep(fresh, S, idx=small)
    finally:
        fresh.close()
    assert np.array_equal(got, want), (note, rel_err(got, want))
    assert (big != 0).any(), note


def interpolmolext(o, gtemp, temp, dens, molidx):
    """extinction.c:535-581 restated in long double: e[layer][wn] and the bound 4 (nmol + 2) eps sum_m |rho_m ext_m|."""
    o = o.astype(np.longdouble); g = gtemp.astype(np.longdouble)
    nl, nt, nm, nw = o.shape
    e = np.zeros((nl, nw), dtype=np.longdouble); mag = np.zeros((nl, nw), dtype=np.longdouble)
    for r in range(nl):
        t = np.longdouble(temp[r])
        it = int(np.searchsorted(gtemp, temp[r], side="right")) - 1
        for m in range(nm):
            ext = (o[r, it, m] * (g[it + 1] - t) + o[r, it + 1, m] * (t - g[it])) / (g[it + 1] - g[it])
            term = np.longdouble(dens[molidx[m], r]) * ext
            e[r] += term; mag[r] += np.abs(term)
    return e, 4 * (nm + 2) * np.finfo(np.float64).eps * mag


def check_grid_run(P, g, o, gtemp, note):
    """One grid-mode run of handle g against the oracle on the same grid, and its extinction against interpolmolext."""
    got = check_against_oracle(P, g, oracle(P), note)
    assert got is not None, note
    L = P.layer_arrays()
    grid = P.static.ogrid.contents
    molidx = [grid.mol_index[m] for m in range(grid.nmol)]
    want, bound = interpolmolext(o.reshape(P.nlayer, len(gtemp), grid.nmol, P.nwn), gtemp, L["temp"], L["density"], molidx)
    sw = got["computed"].astype(bool)
    assert sw.any(), note
    err = np.abs(got["e"][sw].astype(np.longdouble) - want[sw])
    assert (err <= bound[sw]).all(), (note, float((err / np.where(bound[sw] > 0, bound[sw], 1)).max()))
    return got["spectrum"]


@pytest.mark.parametrize("seed", range(NCASES))
def test_random_grid_mode_against_oracle(tmp_path, seed):
    """Build the grid with the HIP sweep; then on one grid-mode handle: the atmosphere as written, moved, on interior
    nodes, at tlow and just below thigh, each against the oracle's grid-mode run; thigh and below tlow refused with
    the handle still usable; a batch of the atmospheres and shards bit for bit the single handle's spectra."""
    P, kw, note = make_problem(tmp_path, seed)
    hip = Engine(P.static)
    try:
        o = hip.build_opacity_grid(P)
    finally:
        hip.close()
    assert P.static.ogrid and not P.needs_opacity_build, note
    e = kw["extra"]
    gtemp = np.arange(e["tlow"], e["thigh"] + 0.5, e["tempdelt"], dtype=float)
    nl = P.nlayer
    temp = np.ctypeslib.as_array(P.atm.temp, shape=(nl,))
    base = temp.copy()
    rng = np.random.default_rng(13000 + seed)
    t_min = max(float(e["tlow"]), [0.0, 400.0, 800.0][kw["ncia"]])        # (inside the CIA tables too)
    t_max = np.nextafter(float(e["thigh"]), 0.0)
    edges = [gtemp[k] for k in range(1, len(gtemp) - 1) if gtemp[k] >= t_min]
    if e["tlow"] >= t_min:
        edges.append(float(e["tlow"]))
    edges.append(t_max)
    atms = {"as written": base.copy(), "moved": rng.uniform(t_min, t_max, nl),
            "on nodes and edges": rng.choice(edges, nl)}
    g = Engine(P.static)
    spectra = {}
    try:
        for name, t in atms.items():
            temp[:] = t
            spectra[name] = check_grid_run(P, g, o, gtemp, (note, name))
        # outside the grid: refused, and the handle goes on
        for bad in (float(e["thigh"]), np.nextafter(float(e["tlow"]), 0.0)):
            temp[:] = base
            temp[int(rng.integers(0, nl))] = bad
            with pytest.raises(EngineError) as ei:
                g.run(P.atm, P.opts)
            assert ei.value.code == -5, (note, bad)                  # TRX_E_RANGE
        temp[:] = base
        again = g.run(P.atm, P.opts)["spectrum"]
        assert np.array_equal(again, spectra["as written"]), note
    finally:
        temp[:] = base
        g.close()
    # a batch of the atmospheres: the single handle's bits
    keep = []
    for t in atms.values():
        a = _abi.TrxAtm()
        C.memmove(C.byref(a), C.byref(P.atm), C.sizeof(_abi.TrxAtm))
        tt = np.ascontiguousarray(t, dtype=np.float64)
        a.temp = tt.ctypes.data_as(_abi.c_double_p)
        keep.append((a, tt))
    B = Batch(P.static, ways=3)
    try:
        got = B.run([a for a, _ in keep], P.opts)
    finally:
        B.close()
    for j, name in enumerate(atms):
        assert np.array_equal(got[j], spectra[name]), (note, name)
    # shards: slices of the full spectrum
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
                    s = sh.run(P.atm, P.opts)["spectrum"]
                    assert np.array_equal(s, spectra["as written"][lo_:hi_]), (note, lo_, hi_, rep)
            finally:
                sh.close()
    finally:
        P.set_shard(0, nwn)
    SEEN["grid_cases"].add(seed)


def test_random_grid_sweep_reached_its_edges():
    """Coverage is asserted, not assumed: over the seeds the sweeps met a short last step after a full one, walk and
    two-kernel steps in one sweep, the lanes and the packed forms, more than 2 slots, more than 64 isotopes, a slot
    without lines and 2000+ states."""
    if len(SEEN["sweep_cases"]) < NCASES or len(SEEN["grid_cases"]) < NCASES:
        pytest.skip("the random grid sweeps did not run in full in this session")
    counts = {k: len(v) for k, v in SEEN.items() if k not in ("sweep_cases", "grid_cases", "switches")}
    print("random grid sweep: %d seeds, %s, switches %s" % (NCASES, counts, " ".join(SEEN["switches"])))
    for k in counts:
        assert counts[k] >= 1, counts
