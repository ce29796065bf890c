"""libtransit.so on the GPU, driven from C (tests/libtransit_driver.c) as a retrieval driver drives
the reference's library: spectra through reloads and setters, the files every run_transit writes,
the life cycle of the one state, and the opacity-grid path of transit_init."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from cases import GOLDEN, rel_err
from host_check import build_driver, copy_case, probes, run_driver
from transit_amd import build

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
# the reentry goldens: case -> tolerance against the reference's values (as test_reentry.py)
CASES = {"reentry": 1e-9, "reentry_transit": 1e-8, "reentry_set": 1e-9, "reentry_set_transit": 1e-8}
FILES = {"reentry": "eclipse", "reentry_transit": "transit"}     # tests/golden/reentry_files/<name>


def script_of(case):
    with open(os.path.join(GOLDEN, case, "reentry_inputs.txt")) as f:
        return "init case.cfg\n" + f.read() + "free\n"


def module_outputs(work, case):
    """The same script through transit_amd.transit_module in this process, cwd = a copy of the case."""
    import transit_amd.transit_module as trm
    old = os.getcwd()
    os.chdir(str(work))
    outs = []
    try:
        argv = ["transit", "-c", "case.cfg"]
        trm.transit_init(len(argv), argv)
        n = trm.get_no_samples()
        for ln in open(os.path.join(GOLDEN, case, "reentry_inputs.txt")):
            w = ln.split()
            if not w:
                continue
            if w[0] == "radius":
                trm.set_radius(float(w[1]))
            elif w[0] == "cloudtop":
                trm.set_cloudtop(float(w[1]))
            elif w[0] == "scattering":
                trm.set_scattering(int(float(w[1])), float(w[2]))
            else:
                outs.append(trm.run_transit(np.array([float(x) for x in w]), n))
    finally:
        trm.free_memory()
        os.chdir(old)
    return outs


@pytest.fixture(scope="module")
def driver_runs(tmp_path_factory):
    """Every reentry case through the driver once: case -> (work dir, outputs, process)."""
    tmp = tmp_path_factory.mktemp("libtransit")
    exe = build_driver(tmp)
    runs = {}
    for case in CASES:
        work = copy_case(tmp, case)
        for f in ("spectrum.dat", "toomuch.dat", "tau.dat", "CIA.dat", "mol_extion.dat"):
            os.remove(work / f)
        p = run_driver(exe, work, script_of(case))
        assert p.returncode == 0, p.stderr
        assert "status" not in p.stdout.replace("probe status", ""), p.stdout
        k, outs = 1, []
        while os.path.exists(work / ("drv_out%d.dat" % k)):
            outs.append(np.loadtxt(work / ("drv_out%d.dat" % k)))
            k += 1
        runs[case] = (work, outs, p)
    return runs


@pytest.mark.parametrize("case", list(CASES))
def test_driver_follows_the_reference_through_reloads_and_setters(driver_runs, case):
    _, outs, _ = driver_runs[case]
    nruns = sum(1 for ln in open(os.path.join(GOLDEN, case, "reentry_inputs.txt")) if ln.split() and ln.split()[0][0] in "0123456789.-")
    assert len(outs) == nruns
    for k, got in enumerate(outs):
        ref = np.loadtxt(os.path.join(GOLDEN, case, "reentry_out%d.dat" % (k + 1)))
        assert got.shape == ref.shape
        assert rel_err(got, ref) < CASES[case], (case, k)


@pytest.mark.parametrize("case", list(CASES))
def test_driver_equals_the_python_module(driver_runs, tmp_path, case):
    """These cases ask for `savefiles yes`: the library runs them eagerly (every layer swept, for the
    dumps), transit_module does not, so the two are compared at 1e-12 rather than bit for bit."""
    _, outs, _ = driver_runs[case]
    mod = module_outputs(copy_case(tmp_path, case), case)
    assert len(mod) == len(outs)
    for k, (a, b) in enumerate(zip(outs, mod)):
        assert a.shape == b.shape
        assert rel_err(a, b) < 1e-12, (case, k)


@pytest.mark.parametrize("case", list(FILES))
def test_every_run_writes_the_reference_s_files(driver_runs, case):
    """After the three runs, the files left are the reference library driver's after the same script
    (tests/golden/reentry_files, from the compiled reference): tolerances as tests/test_cli.py."""
    work, _, _ = driver_runs[case]
    refdir = os.path.join(GOLDEN, "reentry_files", FILES[case])
    ref_txt = open(os.path.join(refdir, "spectrum.dat")).read().split("\n")
    got_txt = open(work / "spectrum.dat").read().split("\n")
    assert got_txt[0] == ref_txt[0] and len(got_txt) == len(ref_txt)
    got, ref = ol.read_spectrum(work / "spectrum.dat"), ol.read_spectrum(os.path.join(refdir, "spectrum.dat"))
    assert np.array_equal(got[:, 0], ref[:, 0])
    assert rel_err(got[:, 1], ref[:, 1]) < 2e-8
    g = np.loadtxt(work / "toomuch.dat", comments="#", skiprows=2)
    r = np.loadtxt(os.path.join(refdir, "toomuch.dat"), comments="#", skiprows=2)
    assert np.array_equal(g[:, 3], r[:, 3])
    assert rel_err(g[:, 1], r[:, 1]) < 1e-5
    for name, key in (("tau.dat", "wavenumber"), ("CIA.dat", "wavenumber"), ("mol_extion.dat", "radius")):
        ref_path = os.path.join(refdir, name)
        got_lines = open(work / name).read().split("\n")
        ref_lines = open(ref_path).read().split("\n")
        assert got_lines[:4] == ref_lines[:4], name
        assert len(got_lines) == len(ref_lines), name
        gk, gv = ol.read_rows_dump(work / name, key)
        rk, rv = ol.read_rows_dump(ref_path, key)
        assert np.array_equal(gk, rk), name
        assert np.array_equal(gv == 0, rv == 0), name
        assert rel_err(gv, rv) < 1e-8, name


def test_life_cycle_in_one_process(tmp_path):
    """init eclipse -> run -> free -> init transit -> run -> free -> free; init twice; samples after free."""
    exe = build_driver(tmp_path)
    work = copy_case(tmp_path, "reentry", "both")
    shutil.copy(os.path.join(GOLDEN, "reentry_transit", "case.cfg"), work / "transit.cfg")   # same input files
    vec = open(os.path.join(GOLDEN, "reentry", "reentry_inputs.txt")).readline()
    script = ("init case.cfg\n" + vec + "free\ninit transit.cfg\n" + vec + "free\nfree\nprobe\n"
              "init case.cfg\ninit case.cfg\n" + vec + "probe\nfree\nprobe\n")
    p = run_driver(exe, work, script)
    assert p.returncode == 0, p.stderr
    assert "status" not in p.stdout.replace("probe status", ""), p.stdout
    ecl = np.loadtxt(os.path.join(GOLDEN, "reentry", "reentry_out1.dat"))
    tra = np.loadtxt(os.path.join(GOLDEN, "reentry_transit", "reentry_out1.dat"))
    out = [np.loadtxt(work / ("drv_out%d.dat" % k)) for k in (1, 2, 3)]
    assert rel_err(out[0], ecl) < 1e-9
    assert rel_err(out[1], tra) < 1e-8
    assert np.array_equal(out[2], out[0])                  # init twice without free: the same spectrum
    after_free, initialised, freed = probes(p.stdout)
    assert after_free[:2] == (0, 0) and freed[:2] == (0, 0)
    assert initialised[0] == 0 and initialised[1] == ecl.size and initialised[2][0] == 2500.0


def _grid_case(tmp_path, name):
    """opacity_grid with the reload options of reentry/case.cfg appended, its grid file removed."""
    work = copy_case(tmp_path, "opacity_grid", name)
    for f in ("opac.dat", "spectrum.dat"):
        if os.path.exists(work / f):
            os.remove(work / f)
    extra = [ln for ln in open(os.path.join(GOLDEN, "reentry", "case.cfg"))
             if ln.split() and ln.split()[0] in ("refpress", "gsurf", "refradius")]
    with open(work / "case.cfg", "a") as f:
        f.write("".join(extra))
    return work


def _atm_vector(work):
    """[T, q_0, ..., q_{nmol-1}] of the case's own atmosphere file (the reload grammar)."""
    rows, data = open(work / "case.atm").read().split("\n"), []
    start = next(i for i, ln in enumerate(rows) if ln.startswith("#TEADATA"))
    for ln in rows[start + 1:]:
        if ln.strip() and not ln.startswith("#"):
            data.append([float(x) for x in ln.split()])
    a = np.array(data)
    return np.concatenate([a[:, 2]] + [a[:, 3 + j] for j in range(a.shape[1] - 3)])


def test_transit_init_builds_the_opacity_grid(tmp_path):
    exe = build_driver(tmp_path)
    lib = _grid_case(tmp_path, "lib")
    vec = _atm_vector(lib)
    line = " ".join("%.17g" % x for x in vec) + "\n"
    p = run_driver(exe, lib, "init case.cfg\n" + line)
    assert p.returncode == 0, p.stderr
    assert "status" not in p.stdout, p.stdout
    # the grid file is the CLI's, byte for byte
    cli = _grid_case(tmp_path, "cli")
    c = subprocess.run([build.lib_path("transit_hip"), "-c", "case.cfg"], cwd=str(cli), capture_output=True,
                       text=True, timeout=600)
    assert c.returncode == 0, c.stderr
    assert open(lib / "opac.dat", "rb").read() == open(cli / "opac.dat", "rb").read()
    # the spectrum is transit_module's for the same vector (grid file now present: read, not built)
    import transit_amd.transit_module as trm
    old = os.getcwd()
    os.chdir(str(cli))
    try:
        argv = ["transit", "-c", "case.cfg"]
        trm.transit_init(len(argv), argv)
        mod = trm.run_transit(vec, trm.get_no_samples())
    finally:
        trm.free_memory()
        os.chdir(old)
    got = np.loadtxt(lib / "drv_out1.dat")
    assert got.shape == mod.shape and np.all(np.isfinite(got))
    assert rel_err(got, mod) < 1e-12                       # (savefiles: the library's run is eager, the module's not)
    # --justOpacity: initialised, but a run leaves out alone and writes no spectrum
    jo = _grid_case(tmp_path, "just")
    p = run_driver(exe, jo, "init case.cfg --justOpacity\nprobe\n" + line + "probe\n")
    assert p.returncode == 0, p.stderr
    first, second = probes(p.stdout)
    assert first[0] == 0 and first[1] > 0 and second[0] == 0
    out = np.loadtxt(jo / "drv_out1.dat")
    assert out.size == first[1] and np.all(out == SENTINEL)
    assert os.path.exists(jo / "opac.dat") and not os.path.exists(jo / "spectrum.dat")
