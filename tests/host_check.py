"""The build of a stand-alone host check program (tests/<name>.cpp): one compile line under the sanitizers for every
test_*_host.py that runs one.  A plain module -- the fixtures that call it stay with their tests."""
import os
import shutil
import subprocess

import pytest

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
