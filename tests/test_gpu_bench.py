"""bench.py's own contract: a plain run prints the headline alone, --dump-outputs writes the spectrum of the
last timed step (the same for the same arguments, and for one rank or two), and --full adds the secondary
measurements on the same spectrum."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cases import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--lines", "30000", "--layers", "40", "--wnhigh", "2700"]
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"}


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *SMALL, *extra], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_spectrum(tmp_path):
    runs = [_bench("--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path / k)) for k in ("a", "b")]
    for out in runs:
        assert HEADLINE <= set(out)
        assert out["steps"] == 4 and out["warmup"] == 1 and out["ms_per_step"] > 0
        assert out["higher_is_better"] is True and out["dtype"] == "f64"
        c = out["config"]
        assert c["n_wn"] == 201 and 0 < c["layers_needed"] <= 40
        assert out["value"] == pytest.approx(c["n_wn"] * c["layers_needed"] / (out["ms_per_step"] * 1e-3))
        assert "roofline" not in out and "cpu_baseline" not in out and "ms_per_step_steady" not in out
    a, b = (np.load(tmp_path / k / "spectrum.npy") for k in ("a", "b"))
    assert a.dtype == np.float64 and a.shape == (201,)
    assert np.all(np.isfinite(a)) and np.any(a != 0)
    assert np.array_equal(a, b)                         # same arguments, same inputs, same spectrum
    assert not os.path.exists(tmp_path / "a" / "spectrum_index.npy")


@pytest.mark.gpu
def test_full_run_adds_the_secondary_measurements(tmp_path):
    plain = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain"))
    full = _bench("--steps", "3", "--warmup", "1", "--full", "--dump-outputs", str(tmp_path / "full"))
    assert HEADLINE <= set(full) and full["steps"] == 3
    assert {"roofline", "cpu_baseline", "ms_per_step_steady", "ms_per_step_device_spectrum"} <= set(full)
    assert {"ms_kernels", "ms_create_total", "ms_per_spectrum_batch8"} <= set(full["config"])
    assert full["config"]["layers_needed"] == plain["config"]["layers_needed"]
    assert np.array_equal(np.load(tmp_path / "plain" / "spectrum.npy"), np.load(tmp_path / "full" / "spectrum.npy"))


@pytest.mark.gpu
def test_plain_two_rank_run_dumps_the_stitched_spectrum(tmp_path):
    """N > 1 without --full (two ranks sharing the GPU, --rehearse): the headline alone, and rank 0 dumps the
    stitched spectrum -- in eclipse geometry the one-rank spectrum, bit for bit."""
    _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "one"))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "3", "--warmup", "1", "--rehearse", *SMALL, "--dump-outputs", str(tmp_path / "two")]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert HEADLINE <= set(out) and out["n_gpus"] == 2 and out["steps"] == 3
    assert "roofline" not in out and "per_rank" not in out["config"]
    assert np.array_equal(np.load(tmp_path / "one" / "spectrum.npy"), np.load(tmp_path / "two" / "spectrum.npy"))
