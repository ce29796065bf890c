"""The launch decisions of a line-sweep step, on the CPU: transit_amd/csrc/trx_sweep.h (the ranges a shard's walk
launches, the lines its two-kernel form launches, the walk's form, the frame ladder and the wide layers' masks) held
against plain counts by tests/sweep_check.cpp, a stand-alone program built under the address and undefined-behaviour
sanitizers.  Nothing here is loaded into Python."""
import re
import subprocess

import pytest

from host_check import build_check

MUTATIONS = {1: "khi one cell short", 2: "the straddling range dropped", 3: "gz without the below-cell-0 case",
             4: "very_wide from 63 bins"}


def build(tmp, mutation):
    return build_check("sweep_check", tmp, public_headers=False, defines=["SWEEP_MUTATION=%d" % mutation],
                       exe_name="sweep_check_%d" % mutation)


def test_launch_decisions_equal_the_plain_counts(tmp_path):
    """400 seeded group tables (1 to 4 isotope blocks, one empty; nwn 8 to 200; 1 to 4 groups per range; 0 to 60 groups
    per block in descending cells, some below cell 0 and past the last cell) under every kind of window and Rc 0, 1, 3, 7:
    walk_window launches every range with a group in reach, one contiguous run per block with at most one range at
    each end that holds none, the straddling range included, seg_cum the running sum, "nothing reaches" one empty
    segment; sweep_window_lines equals the cell-by-cell count; the ladders at every boundary; walk_form over every
    combination of its inputs.  The draws reach the edge cases they are there for."""
    out = subprocess.run([build(tmp_path, 0), "400"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert re.search(r"^\d+ cases, 0 differ$", out.stdout, re.M), out.stdout
    assert re.search(r"^ok \d+$", out.stdout, re.M), out.stdout
    m = re.search(r"\((\d+) windows: (\d+) ranges straddling one, (\d+) with nothing in reach, (\d+) groups below cell 0 in "
                  r"reach; gaps: (\d+) between two ranges, (\d+) inside one\)", out.stdout)
    assert m and all(int(x) > 100 for x in m.groups()), out.stdout


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_planted_mutation_is_caught(tmp_path, mutation):
    """The header stated wrongly (trx_sweep.h, -DSWEEP_MUTATION): each must fail the check."""
    out = subprocess.run([build(tmp_path, mutation), "400"], capture_output=True, text=True)
    assert out.returncode == 1, (MUTATIONS[mutation], out.stdout, out.stderr)
    assert re.search(r"^\d+ cases, [1-9]\d* differ$", out.stdout, re.M), (MUTATIONS[mutation], out.stdout)
