"""The build of a stand-alone host check program (tests/<name>.cpp): one compile line under the sanitizers for every
test_*_host.py that runs one.  A plain module -- the fixtures that call it stay with their tests."""
import os
import shutil
import subprocess

import pytest

from cases import GOLDEN
from transit_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZED = ["-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build_check(name, out_dir, public_headers=True, defines=(), exe_name=None):
    """tests/<name>.cpp built into out_dir (as exe_name, or name) against transit_amd/csrc -- and include/ unless the
    program takes no public header -- with -D for each of `defines`; skips the caller where there is no g++"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = os.path.join(str(out_dir), exe_name or name)
    headers = (["-I", os.path.join(ROOT, "include")] if public_headers else []) + ["-I", os.path.join(ROOT, "transit_amd", "csrc")]
    subprocess.run([gxx, *SANITIZED, *["-D" + d for d in defines], *headers, "-o", exe, os.path.join(ROOT, "tests", name + ".cpp")], check=True)
    return exe


# ---- libtransit.so's C driver (tests/libtransit_driver.c) ------------------------------------------------------------
INCLUDE = os.path.join(ROOT, "include")
DRIVER = os.path.join(ROOT, "tests", "libtransit_driver.c")


def build_driver(directory) -> str:
    """The test driver, compiled against the header and linked with -ltransit alone."""
    lib = build.build_lib()
    exe = os.path.join(str(directory), "libtransit_driver")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, DRIVER, "-o", exe,
                    "-L", os.path.dirname(lib), "-ltransit", "-Wl,-rpath," + os.path.dirname(lib)],
                   check=True, capture_output=True, text=True, timeout=120)
    return exe


def run_driver(exe, work, script, timeout=600):
    """Runs the driver on `script` (text) in `work`; run k's out goes to work/drv_out<k>.dat."""
    with open(os.path.join(str(work), "script.txt"), "w") as f:
        f.write(script)
    return subprocess.run([exe, "script.txt", "drv_out"], cwd=str(work), capture_output=True, text=True,
                          timeout=timeout)


def copy_case(tmp_path, case, name=None):
    work = tmp_path / (name or case)
    shutil.copytree(os.path.join(GOLDEN, case), work)
    return work


def probes(stdout):
    """The driver's probe lines: (status, samples, wn[3], out0)."""
    out = []
    for ln in stdout.splitlines():
        w = ln.split()
        if w and w[0] == "probe":
            out.append((int(w[2]), int(w[4]), [float(x) for x in w[6:9]], float(w[10])))
    return out
