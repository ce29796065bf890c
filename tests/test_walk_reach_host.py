"""The reach bound of a line range and the whole-range exit of k_line_walk, on the CPU: the kernel's start-up
arithmetic lives in transit_amd/csrc/hip/trx_device.h as host/device functions, and tests/reach_check.cpp holds
them against brute force over every group, layer and slot of seeded random tables, layers and ranges."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MUTATIONS = {1: "bound from the range's last anchor", 2: "sticky profile left out",
             3: "<= for < at the zone's edges", 4: "exit allowed when cell0 != cell1"}


def build(tmp, mutation):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp / ("reach_check_%d" % mutation))
    subprocess.run([gxx, "-O2", "-Wall", "-DREACH_MUTATION=%d" % mutation, "-I", os.path.join(ROOT, "transit_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "reach_check.cpp")], check=True)
    return exe


def test_no_skipped_group_and_no_exited_range_is_within_reach(tmp_path):
    """400 seeded cases (bands spanning a factor of 1.1 to 10, monotone tables and not, steps of 1 to 64 layers,
    wcut inside, above and below the band and on an anchor, osamp 8 to 70000): nothing the bound skips and no range
    an exit accepts can reach a bin with the profile the kernel would select; the bound never exceeds the step's;
    only one-cell ranges exit.  The demo-shaped draw reproduces the shares the change was argued from: about 0.66
    of the groups evaluated under the step's bound, about 0.5 under the range's, about a quarter of the ranges gone."""
    out = subprocess.run([build(tmp_path, 0), "400"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert "400 cases, 0 differ" in out.stdout
    m = re.search(r"\((\d+) groups in (\d+) ranges, (\d+) ranges exited, (\d+) tables not monotone\)", out.stdout)
    assert m and int(m.group(3)) > 1000 and int(m.group(4)) > 20, out.stdout          # the draws reach both paths
    d = re.search(r"evaluated ([\d.]+) under the step's bound, ([\d.]+) under the range's; ranges exited ([\d.]+) by the "
                  r"step's bound, ([\d.]+) in all", out.stdout)
    assert d, out.stdout
    step, rng, exit1, exits = (float(x) for x in d.groups())
    assert 0.60 < step < 0.72 and rng < step - 0.1 and exit1 < exits and 0.15 < exits < 0.40, out.stdout


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_planted_mutation_is_caught(tmp_path, mutation):
    """The start-up restated wrongly (tests/reach_check.cpp, -DREACH_MUTATION): each must fail the check."""
    out = subprocess.run([build(tmp_path, mutation), "400"], capture_output=True, text=True)
    assert out.returncode == 1, (MUTATIONS[mutation], out.stdout)
    assert re.search(r"400 cases, [1-9]\d* differ", out.stdout), (MUTATIONS[mutation], out.stdout)
