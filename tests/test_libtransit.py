"""libtransit.so, the reference's library interface (include/transit_lib.h), driven from C by
tests/libtransit_driver.c: the symbols it exports, the header, the prototypes against the
reference's, and what it does when it cannot initialise."""
import os
import re
import subprocess

import numpy as np
import pytest

from cases import GOLDEN
from host_check import INCLUDE, build_driver, copy_case, probes, run_driver
from transit_amd import build

# where oracle/Makefile finds the reference's sources (its REF)
REF_TRANSIT_C = os.path.join(os.environ.get("REF", "/root/reference"), "transit", "src", "transit.c")

API = ["transit_init", "get_no_samples", "get_waveno_arr", "set_radius", "set_cloudtop", "set_scattering",
       "run_transit", "free_memory"]
EXTRA = ["transit_status", "transit_error"]
TRX_E_NODEVICE = -4


def test_library_exports_exactly_the_ten_functions():
    lib = build.build_lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    names = sorted(ln.split()[-1] for ln in nm.splitlines() if ln.strip())
    assert names == sorted(API + EXTRA)


def test_header_compiles_as_c99_and_as_cpp(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "transit_lib.h"\nint main(void) { return transit_status(); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-fsyntax-only",
                    str(src)], check=True, timeout=60)
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-fsyntax-only",
                    "-x", "c++", str(src)], check=True, timeout=60)


def test_driver_links_with_ltransit_alone(tmp_path):
    exe = build_driver(tmp_path)
    needed = subprocess.run(["readelf", "-d", exe], check=True, capture_output=True, text=True).stdout
    libs = re.findall(r"\(NEEDED\).*\[(.*)\]", needed)
    assert "libtransit.so" in libs
    assert not any(n.startswith(("libtransit_host", "libtransit_hip", "libamdhip")) for n in libs)


def _prototypes(text):
    """name -> (return type, [parameter types]) of the first declaration or definition of each function."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for name in API:
        m = re.search(r"(\w+)\s*(\**)\s*\b" + name + r"\s*\(([^)]*)\)\s*[;{]", text)
        assert m, name
        params = []
        for p in m.group(3).split(","):
            p = " ".join(p.replace("*", " * ").split())
            toks = p.split()
            if len(toks) > 1 and re.match(r"^\w+$", toks[-1]) and toks[-1] not in ("void", "int", "double", "char"):
                toks = toks[:-1]                              # drop the parameter name
            params.append("".join(t if t == "*" else " " + t for t in toks).strip())
        out[name] = (m.group(1) + m.group(2), params)
    return out


def test_prototypes_are_the_reference_s():
    if not os.path.exists(REF_TRANSIT_C):
        pytest.skip("the reference's transit.c is not on this machine")
    with open(REF_TRANSIT_C) as f:                         # declarations at transit.c:14-22 (free_memory: its definition)
        ref = _prototypes(f.read())
    with open(os.path.join(INCLUDE, "transit_lib.h")) as f:
        ours = _prototypes(f.read())
    assert ours == ref
    assert ours["run_transit"] == ("void", ["double*", "int", "double*", "int"])


def test_missing_cfg_fails_without_ending_the_process(tmp_path):
    exe = build_driver(tmp_path)
    work = copy_case(tmp_path, "reentry")
    vec = open(os.path.join(GOLDEN, "reentry", "reentry_inputs.txt")).readline()
    p = run_driver(exe, work, "init nosuch.cfg\nprobe\n" + vec + "probe\n", timeout=120)
    assert p.returncode == 0, p.stderr                      # a normal exit: no exit()/abort() inside
    assert "nosuch.cfg" in p.stderr
    assert len([ln for ln in p.stderr.splitlines() if "nosuch.cfg" in ln]) == 1
    first, second = probes(p.stdout)
    assert first[0] < 0 and first[1] == 0 and first[2] == [-1.0, -1.0, -1.0]
    assert np.isnan(second[3])
    out = np.loadtxt(work / "drv_out1.dat")
    assert out.size == 4 and np.all(np.isnan(out))
    assert not os.path.exists(work / "spectrum.dat") or open(work / "spectrum.dat").read() == \
        open(os.path.join(GOLDEN, "reentry", "spectrum.dat")).read()


def test_no_device_gives_nodevice_and_a_normal_exit(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    exe = build_driver(tmp_path)
    work = copy_case(tmp_path, "reentry")
    p = run_driver(exe, work, "init case.cfg\nprobe\n", timeout=120)
    assert p.returncode == 0, p.stderr
    (status, samples, wn, _), = probes(p.stdout)
    assert status == TRX_E_NODEVICE and samples == 0 and wn == [-1.0, -1.0, -1.0]
    assert "trx_create failed" in p.stderr
