"""The plan of the RANSAC scoring step (putslam_amd/csrc/ps_score_plan.h: staged or complete scoring, the launches and arena blocks of a
call, the "nothing to gain" policy's state machine) compiled into a plain C++ program -- no HIP header, no GPU -- and run
(tests/cpp/test_score_plan.cpp): the state machine against its documented rule; every decision against what the code decided before it
moved into the header (tests/golden/score_plan_parent.json, recorded from the parent commit: tests/golden/make_score_plan_parent.py);
the match ranges of the kernels' work-groups and wavefronts against their tiling properties and their earlier expressions;
the cost model against the rows the GPU tests run (tests/score_plan_rows.py)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_plan_rows as R  # noqa: E402


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("score_plan") / "test_score_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "putslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_score_plan.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(ROOT, "tests", "golden", "score_plan_parent.json")) as f:
        doc = json.load(f)
    # the fixture's columns are the ones this test reads it with
    assert (tuple(doc["input_fields"]), tuple(doc["head_fields"]), tuple(doc["decision_fields"]), tuple(doc["blocks"]), tuple(doc["schedule_fields"]),
            tuple(doc["launch_fields"])) == (R.INPUT_FIELDS, R.HEAD_FIELDS, R.DECISION_FIELDS, R.BLOCKS, R.SCHEDULE_FIELDS, R.LAUNCH_FIELDS)
    return [(dict(zip(R.INPUT_FIELDS, row["in"])), row["out"]) for row in doc["rows"]]


def _run(exe, mode, text):
    run = subprocess.run([exe] + ([mode] if mode else []), input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    return run.stdout


def test_bail_tracker_holds_the_documented_rule(program):
    assert _run(program, None, "").strip() == "score plan ok"


def test_match_ranges_tile_and_equal_the_parent_commit(program):
    """pair_split, stage_range, group_part and wave_part (the range arithmetic of ps_score_pass.h's pass_begin): the stages tile [0, M),
    the work-group and wavefront parts tile every stage range in blocks of 64, the pair split tiles [0, M) in even parts -- over M = 0 ..
    600 and PS_MAX_KPTS, every best0, msplit = 1 .. 32, both orders, both granularities, every list_cover -- and each equals the
    expressions the kernels held before the arithmetic moved into the header (restated in the program)."""
    assert _run(program, "ranges", "").strip() == "match ranges ok"


def test_the_parent_table_covers_every_decision(parent):
    assert len(parent) >= 200
    cov = R.coverage([(r_in, R.parse_output(out)) for r_in, out in parent])
    assert all(cov.values()), [name for name, seen in cov.items() if not seen]


def test_every_decision_equals_the_parent_commit(program, parent):
    lines = _run(program, "plan", "".join(R.input_line(r_in) + "\n" for r_in, _ in parent)).splitlines()
    assert len(lines) == len(parent)
    for (r_in, out), line in zip(parent, lines):
        got = [int(x) for x in line.split()]
        assert got == out, (r_in, R.parse_output(out), R.parse_output(got))


def test_cost_model_rows_on_the_host(program):
    """The rows of tests/test_gpu_prune.py::test_cost_model_*: complete scoring with `below` pairs, the staged form with `above`; side by
    side rows also hold that a lone context scores completely on either side of the point."""
    asked, expect = [], []
    for mode, est, H, kpts, below, above in R.COST_MODEL_ROWS:
        for P, staged in ((below, 0), (above, 1)):
            asked.append((R.family_of(mode), est, H, kpts, P, 0))
            expect.append(staged)
    for mode, est, H, kpts, sbs, below, above in R.COST_MODEL_SBS_ROWS:
        for P, staged in ((below, 0), (above, 1)):
            asked += [(R.family_of(mode), est, H, kpts, P, sbs), (R.family_of(mode), est, H, kpts, P, 0)]
            expect += [staged, 0]
    got = [int(x) for x in _run(program, "staged", "".join(" ".join(map(str, a)) + "\n" for a in asked)).split()]
    assert got == expect, [a for a, g, e in zip(asked, got, expect) if g != e]
