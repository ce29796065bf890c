"""The CPU oracle against the compiled reference on the seeded opacity-grid problems
(random_cases.random_grid_case): the grid file calcopacity() writes (opacity.c:282-427) and the
grid-mode spectrum (interpolmolext, extinction.c:535-581), on the same seeds on which
test_gpu_grid_random.py holds the HIP sweep and the grid-mode runs to the oracle.  The reference
runs in the case directory (oracle/_ref/transit) and writes the grid; the oracle then builds its
own from the same inputs.  Skipped where the reference is not built.

Isotopes without lines get one weak line each (random_cases.fill_empty_isotopes), as in
test_random_reference.py: the reference cannot read them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import random_cases
from cases import rel_err
from tolerances import DEBUG_KEYS, assert_tau_close
from transit_amd import synth
from transit_amd.engine import EngineError
from transit_amd.host import Problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
NCASES = int(os.environ.get("TRX_RANDOM_GRID_REF_CASES", "48"))


@pytest.mark.parametrize("seed", range(NCASES))
def test_oracle_grid_against_the_reference_binary(tmp_path, seed):
    exe = os.path.join(REF_DIR, "transit")
    if not (os.path.exists(exe) and os.access(exe, os.X_OK)):
        pytest.skip("%s is not built (needs the reference sources at build time)" % os.path.relpath(exe, ROOT))
    kw = random_cases.fill_empty_isotopes(random_cases.random_grid_case(seed))
    note = random_cases.summary(kw)
    d = str(tmp_path / "g")
    synth.make_case(d, **kw)
    p = subprocess.run([exe, "-c", "case.cfg"], cwd=d, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (note, p.stderr[-2000:])
    shutil.move(os.path.join(d, "opac.dat"), os.path.join(d, "opac_ref.dat"))
    P = Problem.from_cfg(os.path.join(d, "case.cfg"))
    assert P.needs_opacity_build, note
    ora = ol.OracleEngine(P.static)
    try:
        o = ora.build_opacity_grid(P)
    finally:
        ora.close()
    ids, temp, press, wns, og = ol.read_grid(os.path.join(d, "opac.dat"))
    rids, rtemp, rpress, rwns, rog = ol.read_grid(os.path.join(d, "opac_ref.dat"))
    e = kw["extra"]
    assert np.array_equal(temp, np.arange(e["tlow"], e["thigh"] + 0.5, e["tempdelt"], dtype=float)), note
    assert np.array_equal(ids, rids) and np.array_equal(temp, rtemp) and np.array_equal(wns, rwns), note
    # (the header's pressures: the reference writes the ones it resampled onto its radius grid (up to 2.5e-9 off
    # the file's at the top of a 3-layer atmosphere), the host the file's own.  The values below hold to 1e-9.)
    assert rel_err(press, rpress) < 1e-8, note
    assert og.shape == rog.shape and og.shape[2] == len(kw["dbs"]), (note, og.shape, rog.shape)
    assert np.array_equal(og.reshape(o.shape), o), note
    assert np.array_equal(og == 0, rog == 0), note            # same thresholded / untouched bins
    assert (rog != 0).any(), note
    assert rel_err(og, rog) < 1e-9, note
    # the grid-mode spectrum (the reference ran it on its own grid, the oracle runs it on its own)
    ora = ol.OracleEngine(P.static)
    try:
        out = ora.run(P.atm, P.opts, debug=DEBUG_KEYS)
    except EngineError as err:
        raise AssertionError("the oracle refuses what the reference ran: %s; %s" % (err, note))
    finally:
        ora.close()
    ref_spec = np.loadtxt(os.path.join(d, "spectrum.dat"), comments="#", ndmin=2)[:, 1]
    ref_last = np.loadtxt(os.path.join(d, "toomuch.dat"), comments="#", skiprows=2, ndmin=2)[:, 3].astype(np.int64)
    assert len(ref_spec) == P.nwn, note
    assert np.array_equal(out["last"], ref_last), note
    # (the bounds of test_random_reference.py: rays whose optical depth can carry the parabola noise of
    # tests/tolerances.py pass it on -- no tau.dat here, so which rays those are comes from the oracle's own run)
    noisy = assert_tau_close(P, out, out, note)
    assert rel_err(out["spectrum"][~noisy], ref_spec[~noisy]) < 2e-8, note
    assert rel_err(out["spectrum"], ref_spec) < 1e-7, note
