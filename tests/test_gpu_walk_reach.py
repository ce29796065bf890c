"""k_line_walk's reach bound per line range and its whole-range exit (trx_walk.hip.h; TRX_RANGE_REACH=0: the
step's bound, every range walked): the groups and ranges left out would have added kk * 0 in every lane, so
every output and every debug array is the same BITS with and without -- on a list made for it:

  * band 400-800 cm-1 (a factor of two: the Doppler-dominated reach halves along it) in cells of 0.25 cm-1,
    where the upper layers' profiles reach 0.1-0.2 of a cell;
  * main isotope: three clumps of 8 cells with ~600 lines per cell (> 300 co-added groups per cell: ranges of 32
    groups are a tenth of a cell long, many wholly inside the zone no profile reaches) at the band's ends and
    middle;
  * second isotope, sparse: ranges that span many cells; a stretch whose lines all sit mid-cell (both ends of a
    range in the zone, in different cells: never an exit); 32 k + 1 well-separated lines (a one-group last range).

Steps of 64 layers, of the production plan, of 1 layer and 8-bin steps through k_line_walk itself (the lanes and
packed forms switched off), a threshold that drops groups, ragged shards, both geometries, unhinted / hinted /
resumed runs, one queue and two.  The spectrum is also held to the CPU oracle."""
import os

import numpy as np
import pytest

from tolerances import KEYS, assert_same, check_against_oracle, oracle
from transit_amd import engine, synth
from transit_amd.engine import Engine
from transit_amd.host import Problem

pytestmark = pytest.mark.gpu

WNLOW, WNHIGH, WNDELT, OSAMP = 400.0, 800.0, 0.25, 1080
CLUMPS = (402.0, 600.0, 797.0)          # first cell edge of each dense clump (8 cells = 2 cm-1)


def reach_dbs(seed=7):
    rng = np.random.default_rng(seed)
    main = np.concatenate([rng.uniform(c, c + 8 * WNDELT, 8 * 600) for c in CLUMPS])
    # sparse: one line per ~4 cells on a jittered lattice (no two within a fine-grid step: groups = lines) ...
    n_sparse = 32 * 9 + 1
    lattice = np.linspace(WNLOW + 1.0, WNHIGH - 1.0, n_sparse) + rng.uniform(-0.2, 0.2, n_sparse)
    # ... but between 500 and 560 cm-1 every line mid-cell, two per cell (ranges of 32 groups over 16 cells, all in the zone)
    lattice = lattice[(lattice < 500.0) | (lattice > 560.0)]
    cells = 500.0 + WNDELT * np.arange(int(60 / WNDELT))
    mid = np.concatenate([cells + WNDELT * 0.45, cells + WNDELT * 0.55])
    sparse = np.concatenate([lattice, mid])
    sparse = sparse[: len(sparse) - (len(sparse) - 1) % 32]             # 32 k + 1 lines
    assert len(sparse) % 32 == 1
    db = synth.synth_linedb(2, WNLOW, WNHIGH, seed)                     # (isotopes, partition functions: the demo's CH4)
    for k, wn in enumerate((main, sparse)):
        wn = np.sort(wn)[::-1]
        db.wl[k] = 1e4 / wn
        db.elow[k] = rng.uniform(0.0, 6000.0, wn.size)
        db.gf[k] = 10.0 ** rng.uniform(-12.0, -5.0, wn.size)
    return [db], main, sparse


@pytest.fixture(scope="module")
def problems(tmp_path_factory):
    """(nlayers, solution, ethresh) -> Problem, made once each."""
    made = {}

    def get(nlayers, solution, ethresh=1e-50):
        key = (nlayers, solution, ethresh)
        if key not in made:
            d = str(tmp_path_factory.mktemp("reach"))
            dbs, main, sparse = reach_dbs()
            # what the case is for: > 300 lines per cell in the clumps even after co-adding (1080 fine points per cell)
            per_cell = np.histogram(main, bins=np.arange(CLUMPS[0], CLUMPS[0] + 8 * WNDELT + 1e-9, WNDELT))[0]
            fine = np.unique(np.round((main - WNLOW) / (WNDELT / OSAMP)))
            assert per_cell.min() > 500 and fine.size > 400 * 24
            synth.make_case(d, wnlow=WNLOW, wnhigh=WNHIGH, wndelt=WNDELT, wnosamp=OSAMP, nlayers=nlayers, solution=solution,
                            toomuch=10.0, ethresh=ethresh, dbs=dbs, ncia=1)
            made[key] = Problem.from_cfg(os.path.join(d, "case.cfg"))
        return made[key]
    return get


def handles(P, env=None):
    """The default handle and the one with TRX_RANGE_REACH=0 (switches are read by Engine() alone)."""
    out = []
    for val in (None, "0"):
        for k, v in (env or {}).items():
            os.environ[k] = v
        if val is not None:
            os.environ["TRX_RANGE_REACH"] = val
        try:
            out.append(Engine(P.static))
        finally:
            os.environ.pop("TRX_RANGE_REACH", None)
            for k in (env or {}):
                os.environ.pop(k, None)
    return out


def runs_give_the_same_bits(P, env=None, scales=(1.0, 1.0, 0.03, 1.0), note=None):
    """Unhinted, hinted, resumed (the atmosphere thinner under the remembered depth) and hinted again, with every
    debug array; then a production run (finished rays' ranges skipped)."""
    a, b = handles(P, env)
    dens = np.ctypeslib.as_array(P.atm.density, shape=(P.static.nmol * P.nlayer,))
    base = dens.copy()
    last = None
    try:
        for k, sc in enumerate(scales):
            dens[:] = base * sc
            ra, rb = a.run(P.atm, P.opts, debug=KEYS), b.run(P.atm, P.opts, debug=KEYS)
            assert_same(ra, rb, (note, k, sc))
            assert a.stats()["layers_swept"] == b.stats()["layers_swept"]
        dens[:] = base
        ra, rb = a.run(P.atm, P.opts), b.run(P.atm, P.opts)
        assert_same(ra, rb, (note, "production"))
        last = ra
    finally:
        dens[:] = base
        a.close(); b.close()
    return last


def frames_of(P):
    seen = []
    engine.set_log(lambda lvl, m: seen.append(m), 5)
    try:
        e = Engine(P.static)
        e.run(P.atm, P.opts)
        e.close()
    finally:
        engine.set_log(None)
    fr = [m for m in seen if "walk frame (bins) per layer" in m]
    assert fr, "no frame report in the debug log"
    return [int(t) for t in fr[-1].split(":")[-1].split()]


@pytest.mark.parametrize("solution", ["eclipse", "transit"])
@pytest.mark.parametrize("two_queues", ["1", "0"])
def test_64_layer_step_same_bits(problems, solution, two_queues):
    """100 layers: the upper step holds 64 layers of 2-bin frames (the headline's k_line_walk<2>), the deep steps wider
    ones; the second walk on its own queue or behind the first."""
    P = problems(100, solution)
    fr = frames_of(P) if two_queues == "1" else None
    if fr is not None:
        assert fr[:40].count(2) >= 30, fr              # the upper layers reach less than a cell: the zone exists
    runs_give_the_same_bits(P, env={"TRX_TWO_QUEUES": two_queues}, note=(solution, two_queues))


@pytest.mark.parametrize("solution", ["eclipse", "transit"])
def test_against_the_oracle(problems, solution):
    """24 layers, default switches: first and hinted run against the CPU oracle (spectrum 1e-8, optical depth and
    extinction as tests/tolerances.py and test_gpu_random hold every such case)."""
    P = problems(24, solution)
    ref = oracle(P)
    hip = Engine(P.static)
    try:
        for rep in range(2):
            check_against_oracle(P, hip, ref, (solution, rep))
    finally:
        hip.close()
    runs_give_the_same_bits(P, note=solution)


@pytest.mark.parametrize("nlayers,chunk", [(24, 1), (24, 5), (16, 8), (8, 0)])
def test_every_step_through_k_line_walk(problems, nlayers, chunk):
    """Eager sweeps in steps of 1, 5 and 8 layers and a production plan of 8, the lanes and the packed form
    switched off: every frame size (the deep layers' 4-, 8- and 16-bin steps too) runs k_line_walk, one lane per
    layer and two."""
    P = problems(nlayers, "eclipse")
    env = {"TRX_LANES_WALK": "0", "TRX_NO_PACKED_WALK": "1"}
    fr = frames_of(P)
    assert 2 in fr, fr                               # the upper layers reach less than a cell
    P.opts.eager, P.opts.layer_chunk = (1, chunk) if chunk else (0, 0)
    try:
        runs_give_the_same_bits(P, env=env, scales=(1.0, 1.0), note=(nlayers, chunk))
    finally:
        P.opts.eager, P.opts.layer_chunk = 0, 0


def test_threshold_that_drops_groups(problems):
    """ethresh 1e-4: most groups fall below the layer's limit (their weight is zero, their frame moves all the same)."""
    P = problems(24, "eclipse", 1e-4)
    runs_give_the_same_bits(P, note="ethresh")
    runs_give_the_same_bits(P, env={"TRX_LANES_WALK": "0", "TRX_NO_PACKED_WALK": "1"}, scales=(1.0, 1.0), note="ethresh, k_line_walk")


@pytest.mark.parametrize("lo,hi", [(3, 20), (13, 811), (795, 1600), (1589, 1599)])
def test_ragged_shards(problems, lo, hi):
    """Shards that cut a clump's cells, start inside the mid-cell stretch, or hold a few bins of the last clump: only
    the ranges in reach are launched and the slot masks are clipped at the edges."""
    P = problems(24, "eclipse")
    P.set_shard(lo, hi)
    try:
        runs_give_the_same_bits(P, scales=(1.0, 1.0), note=(lo, hi))
        runs_give_the_same_bits(P, env={"TRX_LANES_WALK": "0", "TRX_NO_PACKED_WALK": "1"}, scales=(1.0,), note=(lo, hi, "k_line_walk"))
    finally:
        P.set_shard(0, P.nwn)
