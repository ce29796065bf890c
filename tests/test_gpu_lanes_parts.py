"""k_line_walk_lanes with 2, 3 or 4 lanes per layer in its accumulation phase (TRX_LANES_PARTS caps the number
the host picks from the step's layer count: 4 up to 16 layers, 3 up to 21, else 2).  A lane holds fewer bins
of the frame, the frame and the order of every (layer, bin) sum stay what they were: the same BITS in
extinction, optical depth and spectrum whichever number runs, and the same as k_line_walk
(TRX_LANES_WALK=0).  Steps of 16, 17, 21, 24 and 31 layers (demo-shaped atmospheres, both geometries), a
shard, co-added groups with a threshold that drops some, and 16-bin frames."""
import os
import re

import numpy as np
import pytest

from transit_amd import engine, synth
from transit_amd.engine import Engine
from transit_amd.host import Problem

pytestmark = pytest.mark.gpu

DEBUG = ("e", "tau", "last", "computed")
STEP = re.compile(r"walk: lanes = lines, (\d+) layers, (\d+)-bin frames, (\d+) lanes per layer")


def runs_with(P, env, runs=2):
    """Results of one handle created under env (unhinted and hinted debug runs, a production run), and the
    (layers, frame bins, lanes per layer) of every k_line_walk_lanes step it took."""
    msgs = []
    engine.set_log(lambda lvl, m: msgs.append(m), 5)
    for k, v in env.items():
        os.environ[k] = v
    try:
        e = Engine(P.static)
    finally:
        for k in env:
            os.environ.pop(k, None)
    try:
        res = [e.run(P.atm, P.opts, debug=DEBUG) for _ in range(runs)]
        res.append(e.run(P.atm, P.opts))
        e.close()
    finally:
        engine.set_log(None)
    steps = {tuple(int(g) for g in m.groups()) for m in map(STEP.search, msgs) if m}
    return res, steps


def assert_same(a, b, what):
    for ra, rb in zip(a, b):
        sw = ra["computed"].astype(bool) if "computed" in ra else slice(None)
        for k in ra:
            if k == "e":
                assert np.array_equal(ra[k][sw], rb[k][sw]), (what, k)
            else:
                assert np.array_equal(ra[k], rb[k]), (what, k)


def every_parts(P, runs=2):
    """k_line_walk (the reference) and k_line_walk_lanes capped at 2, 3 and 4 lanes per layer: all the same bits.
    Returns the steps each cap took."""
    ref, _ = runs_with(P, {"TRX_LANES_WALK": "0"}, runs)
    seen = {}
    for parts in ("2", "3", "4"):
        got, steps = runs_with(P, {"TRX_LANES_WALK": "2", "TRX_LANES_PARTS": parts}, runs)
        assert steps, "the lanes form was never taken: the test compares nothing"
        assert all(p == min(int(parts), 4 if nc <= 16 else 3 if nc <= 21 else 2) for nc, _, p in steps), steps
        assert_same(got, ref, "lanes per layer <= %s against k_line_walk" % parts)
        seen[parts] = steps
    return seen


def demo_case(tmp_path, solution, nlayers=100, nlines=120_000, **kw):
    d = str(tmp_path / "c")
    args = dict(nlines=nlines, wnlow=2500, wnhigh=2800, wndelt=1.0, wnosamp=2160, nlayers=nlayers, solution=solution,
                toomuch=10.0, ethresh=1e-50, seed=11, ncia=2 if solution == "transit" else 1)
    args.update(kw)
    synth.make_case(d, **args)
    return Problem.from_cfg(os.path.join(d, "case.cfg"))


@pytest.mark.parametrize("solution", ["eclipse", "transit"])
def test_parts_on_the_demo_plan(tmp_path, solution):
    """The production plan of a demo-shaped atmosphere (unhinted, then hinted: another step plan)."""
    P = demo_case(tmp_path, solution)
    every_parts(P)


def frames_and_plan(P):
    """The walk frame of every layer (top first) of an eager sweep, and plan(c): the (layers, frame) of each walk step
    trx_run makes for layer_chunk = c (equal parts of what is left, the first step at least 3 layers)."""
    seen = []
    engine.set_log(lambda lvl, m: seen.append(m), 5)
    try:
        e = Engine(P.static)
        P.opts.eager, P.opts.layer_chunk = 1, 0
        e.run(P.atm, P.opts)
        e.close()
    finally:
        engine.set_log(None)
    fr = [m for m in seen if "walk frame (bins) per layer" in m]
    assert fr, "no frame report in the debug log"
    frames = [int(t) for t in fr[0].split(":")[-1].split()]

    def plan(c):
        nwalk = frames.index(0) if 0 in frames else len(frames)
        pos, out = 0, []
        while pos < nwalk:
            left = nwalk - pos
            nc = -(-left // -(-left // c))
            if pos == 0:
                nc = max(nc, 3)
            out.append((nc, max(frames[pos:pos + nc])))
            pos += nc
        return out
    return frames, plan


def test_parts_on_the_headline_plan(tmp_path):
    """The headline's own input (bench.py: 10^6 lines, 2500-5000 cm-1): its deep step, 17 layers of 8-bin frames,
    runs with 3 lanes per layer."""
    P = demo_case(tmp_path, "eclipse", nlines=1_000_000, wnhigh=5000, seed=1234)
    seen = every_parts(P, runs=1)
    assert any(nb == 8 and p == 3 and 17 <= nc <= 21 for nc, nb, p in seen["4"]), seen


@pytest.mark.parametrize("solution", ["eclipse", "transit"])
@pytest.mark.parametrize("parts,lo,hi", [(4, 3, 16)])
def test_parts_on_8_bin_frames(tmp_path, solution, parts, lo, hi):
    """k_line_walk_lanes<8> with 4 lanes per layer (a step of at most 16 layers): a step size whose plan has such a
    step with 8-bin frames, against 2 lanes per layer and k_line_walk."""
    P = demo_case(tmp_path, solution, nlines=20_000, wnhigh=2560, seed=91)
    frames, plan = frames_and_plan(P)
    chunk = next((c for c in range(3, 40) if any(fr == 8 and lo <= nc <= hi for nc, fr in plan(c))), None)
    assert chunk is not None, frames
    P.opts.eager, P.opts.layer_chunk = 1, chunk
    seen = every_parts(P, runs=1)
    assert any(nb == 8 and p == parts and lo <= nc <= hi for nc, nb, p in seen["4"]), (chunk, plan(chunk), seen)
    assert any(nb == 8 and p == 2 and lo <= nc <= hi for nc, nb, p in seen["2"]), (chunk, seen)


@pytest.mark.parametrize("solution", ["eclipse", "transit"])
@pytest.mark.parametrize("chunk", [16, 17, 21, 24, 31])
def test_parts_on_steps_of_n_layers(tmp_path, solution, chunk):
    """Eager sweeps in steps of about `chunk` layers (equal parts from the top): the deep steps hold 8- and 16-bin
    frames and take 4, 3 or 2 lanes per layer by their size (every_parts checks which)."""
    P = demo_case(tmp_path, solution)
    P.opts.eager = 1
    P.opts.layer_chunk = chunk
    seen = every_parts(P, runs=1)
    assert max(nc for nc, _, _ in seen["4"]) <= chunk, seen


def test_parts_on_16_bin_frames(tmp_path):
    """Steps of 16 layers reach the 16-bin frames of the deep layers: k_line_walk_lanes<16> with 2, 3 and 4 lanes
    per layer (steps of 21: 3)."""
    P = demo_case(tmp_path, "eclipse", nlines=20_000, wnhigh=2560, seed=91)
    P.opts.eager = 1
    for chunk, want in ((16, 4), (21, 3)):
        P.opts.layer_chunk = chunk
        seen = every_parts(P, runs=1)
        assert any(nb == 16 and p == want for _, nb, p in seen["4"]), seen
        assert any(nb == 16 and p == 2 for _, nb, p in seen["2"]), seen


@pytest.mark.parametrize("chunk", [16, 21])
def test_parts_on_a_shard(tmp_path, chunk):
    """A shard: only the ranges that reach it are launched, blocks of the range at its edges are ragged."""
    P = demo_case(tmp_path, "eclipse")
    P.opts.eager = 1
    P.opts.layer_chunk = chunk
    P.set_shard(37, 211)
    try:
        every_parts(P, runs=1)
    finally:
        P.set_shard(0, P.nwn)


@pytest.mark.parametrize("chunk", [16, 21])
def test_parts_with_coadding_and_threshold(tmp_path, chunk):
    """A coarse fine grid (wnosamp 400: co-added groups of up to ~10 lines) and a threshold that drops groups; eager
    steps of about `chunk` layers (its production plan takes no step of wide frames)."""
    d = str(tmp_path / "c")
    synth.make_case(d, nlines=60_000, wnlow=2500, wnhigh=2560, wndelt=1.0, wnosamp=400, nlayers=60,
                    solution="eclipse", toomuch=10.0, ethresh=1e-4, seed=5)
    P = Problem.from_cfg(os.path.join(d, "case.cfg"))
    P.opts.eager = 1
    P.opts.layer_chunk = chunk
    every_parts(P)
