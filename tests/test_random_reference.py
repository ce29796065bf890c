"""The CPU oracle against the compiled reference on the random sweep's corners (tests/random_cases.py):
the same seeds test_gpu_random.py runs the HIP path on, so that "agrees with the oracle" there means
"agrees with the reference" -- at layer counts around the walk step and the tail's limit, with up to
256 isotopes in 1-3 line databases, 1-16 angles, clouds and scattering.  The reference is run in the
case directory (oracle/_ref/transit, or transit_zinit where the cloud model needs it, as
tests/golden/make_golden.py chooses); skipped where it is not built.

A known hole: isotopes without lines.  The reference reads such an isotope past the end of its line
arrays (readlineinfo.c:496-524), so every case here gives each of them one weak line in the band
(random_cases.fill_empty_isotopes) and the oracle is never pinned to the reference on that corner;
there the GPU sweep leans on the oracle alone, whose host side skips the isotope's lines."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import random_cases
from cases import rel_err
from transit_amd import synth
from transit_amd.engine import EngineError
from transit_amd.host import Problem
from tolerances import DEBUG_KEYS, assert_tau_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")


@pytest.mark.parametrize("seed", range(int(os.environ.get("TRX_RANDOM_REF_CASES", "48"))))
def test_oracle_against_the_reference_binary(tmp_path, seed):
    kw = random_cases.random_case(seed)
    exe = os.path.join(REF_DIR, random_cases.reference_binary(kw))
    if not (os.path.exists(exe) and os.access(exe, os.X_OK)):
        pytest.skip("%s is not built (needs the reference sources at build time)" % os.path.relpath(exe, ROOT))
    note = random_cases.summary(kw)
    d = str(tmp_path / "r")
    kw = random_cases.fill_empty_isotopes(kw)                 # (what the reference can read)
    kw = dict(kw, extra=dict(kw["extra"], savefiles="yes"))
    synth.make_case(d, **kw)
    p = subprocess.run([exe, "-c", "case.cfg"], cwd=d, capture_output=True, text=True, timeout=300)
    P = Problem.from_cfg(os.path.join(d, "case.cfg"))
    ora = ol.OracleEngine(P.static)
    try:
        if p.returncode != 0:
            # a case the reference rejects, the oracle rejects too
            with pytest.raises(EngineError):
                ora.run(P.atm, P.opts, debug=DEBUG_KEYS)
            return
        out = ora.run(P.atm, P.opts, debug=DEBUG_KEYS)
    finally:
        ora.close()
    ref_spec = np.loadtxt(os.path.join(d, "spectrum.dat"), comments="#", ndmin=2)[:, 1]
    ref_last = np.loadtxt(os.path.join(d, "toomuch.dat"), comments="#", skiprows=2, ndmin=2)[:, 3].astype(np.int64)
    assert len(ref_spec) == P.nwn, note
    assert np.array_equal(out["last"], ref_last), note
    # optical depth: what the reference printed (tau.dat, 10 digits) against tests/tolerances.py's allowance
    _, tau = ol.read_rows_dump(os.path.join(d, "tau.dat"), "wavenumber")      # [wn][height]
    assert tau.shape == out["tau"].shape, note
    noisy = assert_tau_close(P, {"tau": tau}, out, note)
    # spectrum: the reference's print precision (test_gpu_reference); rays whose optical depth can carry the
    # parabola noise of tests/tolerances.py pass it on, within the bound test_gpu_random.py gives them
    assert rel_err(out["spectrum"][~noisy], ref_spec[~noisy]) < 2e-8, note
    assert rel_err(out["spectrum"], ref_spec) < 1e-7, note
