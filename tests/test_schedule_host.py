"""The queues and events of a pass, on the CPU: transit_amd/csrc/trx_schedule.h (whether a pass ends in the ray tail;
the pass as a flat list of kernels, waits and records in host issue order) held by tests/schedule_check.cpp, a
stand-alone program built under the address and undefined-behaviour sanitizers, against a transcription of the control
flow the schedule replaced and against the ordering rules stated in that file's head.  Nothing here is loaded into
Python."""
import re
import subprocess

import pytest

from host_check import build_check

MUTATIONS = {1: "the side queue's waits for inputs dropped", 2: "the walk's wait for records_free dropped",
             3: "the wait for cia ahead of the first optical depth dropped", 4: "the join dropped",
             5: "the side tail's wait for walk1 dropped", 6: "walk1 recorded ahead of the main queue's wait for cia",
             7: "tail_steps = 3 with the side queue taking the second walk only"}

COVERAGE = (r"\(tails: (\d+) of one step, (\d+) of two steps on two queues, (\d+) of two steps on one queue; (\d+) passes with "
            r"deferred side work, (\d+) with a two-kernel step between walks, (\d+) grid passes, (\d+) with a wholly saved step; "
            r"resumed behind a tail: (\d+), (\d+), (\d+)\)")


def build(tmp, mutation):
    return build_check("schedule_check", tmp, public_headers=False, defines=["SCHEDULE_MUTATION=%d" % mutation],
                       exe_name="schedule_check_%d" % mutation)


def test_schedule_equals_the_transcription_and_keeps_the_rules(tmp_path):
    """plan_check's 20000 seeded cases under every setting of the tail switches, pipelined or not, vertical or slant rays,
    with and without saved layers, and a resumed pass behind every first pass that stops at a hint: schedule_pass equals
    the transcription of the former control flow op for op, tail_choice the four expressions it replaced, and no ordering
    rule is violated.  The draws reach every shape of schedule more than 100 times."""
    out = subprocess.run([build(tmp_path, 0)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert re.search(r"^\d+ cases, 0 differ$", out.stdout, re.M), out.stdout
    assert re.search(r"^rules: [1-9]\d* checked, 0 violated$", out.stdout, re.M), out.stdout
    assert re.search(r"^ok \d+$", out.stdout, re.M), out.stdout
    m = re.search(COVERAGE, out.stdout)
    assert m and all(int(x) > 100 for x in m.groups()), out.stdout


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_planted_mutation_breaks_a_rule(tmp_path, mutation):
    """The schedule stated wrongly (trx_schedule.h, -DSCHEDULE_MUTATION): the ordering rules alone must report each,
    whatever the comparison with the transcription says."""
    out = subprocess.run([build(tmp_path, mutation), "4000"], capture_output=True, text=True)
    assert out.returncode == 1, (MUTATIONS[mutation], out.stdout, out.stderr)
    assert re.search(r"^rules: \d+ checked, [1-9]\d* violated$", out.stdout, re.M), (MUTATIONS[mutation], out.stdout)
    assert "ok " not in out.stdout
