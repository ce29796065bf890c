"""trx_numerics.h building blocks that replace an operation of the reference by a cheaper
sequence must return that operation's bits (CPU: the header is shared by host and kernels)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quotient_rn_is_the_division(tmp_path):
    """x * (1/d) with two fused residual corrections == x / d, bit for bit: divisors 6, layer
    spacings and 2 step^2 in cm, mantissas next to all-ones; numerators random, exact multiples
    and their neighbours, zero (eclipse.c:66-80 through k_optical_depth_vertical)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "quotient_check")
    try:
        hw_fma = " fma " in open("/proc/cpuinfo").read()
    except OSError:
        hw_fma = False
    subprocess.run([gxx, "-O2", "-ffp-contract=off"] + (["-mfma"] if hw_fma else []) + ["-I", os.path.join(ROOT, "transit_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "quotient_check.cpp")], check=True)
    out = subprocess.run([exe, "20000000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert "20000000 operands, 0 differ" in out.stdout
    assert "1000000 parabolas, 0 differ" in out.stdout      # parab3 == parab3_recip == parab3_chain, bit for bit


def test_threaded_grouping_is_the_sequential_loop(tmp_path):
    """trx_create's co-added groups, cut into pieces and grouped on several threads, and its
    per-bin counts == the one-thread loops of extinction.c:445-462 (tests/groups_check.cpp:
    sparse, grid-dense and over-dense lists, many small isotope blocks, ties, lines out of range)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "groups_check")
    subprocess.run([gxx, "-O2", "-pthread", "-I", os.path.join(ROOT, "transit_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "groups_check.cpp")], check=True)
    out = subprocess.run([exe, "40"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert " 0 differ" in out.stdout


def test_step_plan_holds_what_its_consumers_rely_on(tmp_path):
    """The step plan of a run (transit_amd/csrc/trx_plan.h) on seeded random frame profiles, hints,
    layer_chunk values, eager and opacity-grid modes (tests/plan_check.cpp): the steps of a pass tile the
    layers from the top; every step is one kind, its frame the widest of its layers; layers per step within
    the kind's cap, layer_chunk and the strength buffers; three layers in the first step; last_step on the
    pass's last step alone; a pass planned whole == planned step by step; the tail predicate == one or two
    walk steps to the hint; the per-molecule sweep's steps (plan_sweep_step) tile every layer, one kind each, within
    the kind's cap, the frame the widest of the step's layers."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "plan_check")
    subprocess.run([gxx, "-O2", "-Wall", "-I", os.path.join(ROOT, "transit_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "plan_check.cpp")], check=True)
    out = subprocess.run([exe, "20000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert "20000 cases, 0 differ" in out.stdout


@pytest.fixture(scope="module")
def table_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("table_check") / "table_check")
    subprocess.run([gxx, "-O2", "-Wall", "-I", os.path.join(ROOT, "transit_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "table_check.cpp")], check=True)
    return exe


def test_table_layouts_hold_what_their_readers_rely_on(table_check):
    """The Voigt table's plan and the layouts of its three copies (transit_amd/csrc/trx_table.h) on seeded random
    grids (tests/table_check.cpp): profiles tile the table; aliases share everything with the entry a Doppler row
    above; rows of distinct jobs are disjoint in every copy; the walk's rows, descriptors and the compact rows are
    what the kernels assume; the limits that switch a copy off; the nearest-index thresholds against
    nearest_index itself."""
    out = subprocess.run([table_check, "2000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert "2000 cases, 0 differ" in out.stdout


@pytest.mark.parametrize("case", ["eclipse_small", "coadd_thresh", "midres_os4", "highres_fine"])
def test_table_plan_is_the_oracles(table_check, case):
    """psize, poff, the total and both width grids of trx_table.h's plan == the oracle's table, exactly: goldens
    with osamp 2160, 24, 4 and 1, which between them hold rows of every class and 1270 aliases of 3600 entries."""
    import oracle_lib as ol
    from cases import GOLDEN
    from transit_amd.host import Problem
    P = Problem.from_cfg(os.path.join(GOLDEN, case, "case.cfg"))
    st = P.static
    args = [st.ndop, st.nlor, repr(st.dmin), repr(st.dmax), repr(st.lmin), repr(st.lmax), repr(st.timesalpha),
            repr(st.wn_d), st.osamp, st.nown]
    out = subprocess.run([table_check, "grid"] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    got = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines()}
    ora = ol.OracleEngine(st)
    ps, off, tab = ora.table()
    adop, alor = ora.width_grids()
    ora.close()
    assert int(got["total"][0]) == tab.size
    assert np.array_equal(np.array(got["psize"], dtype=np.int64), ps.ravel())
    assert np.array_equal(np.array(got["poff"], dtype=np.int64), off.ravel())
    assert np.array_equal(np.array([float.fromhex(x) for x in got["adop"]]), adop)
    assert np.array_equal(np.array([float.fromhex(x) for x in got["alor"]]), alor)
