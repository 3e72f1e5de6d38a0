"""The pipelined stream's ledger and result layout (putslam_amd/csrc/ps_stream_ledger.h: places, staging-area rotation, ring cursor,
pair numbering, epochs; the result block of a chunk) compiled into a plain C++ program -- no HIP header, no GPU -- and run
(tests/cpp/test_stream_ledger.cpp): 24 000 seeded call sequences beside a model of the chunks alive, and, where no chunk fails,
step by step against the expressions ps_stream_async.h held before the ledger (restated in the program)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stream_ledger") / "test_stream_ledger")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "putslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_stream_ledger.cpp"), "-o", exe])
    return exe


def _run(exe, *args):
    run = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    return run.stdout


def test_the_ledger_header_needs_no_hip():
    with open(os.path.join(ROOT, "putslam_amd", "csrc", "ps_stream_ledger.h")) as f:
        includes = re.findall(r'^#include\s+[<"]([^>"]+)[>"]', f.read(), re.M)
    assert includes and not [i for i in includes if "hip/" in i or i.startswith("ps_")], includes


def test_reuse_invariants_and_the_parent_commit_over_random_call_sequences(program):
    """What a new chunk is handed -- staging area and upload event, ring slots, place -- is read by no chunk alive, as its own or as
    its previous frame; places are taken and freed in order; room() is the number of free places; pair numbers and epochs follow
    include/putslam_hip.h across reset and abort; and on the sequences without a failing chunk the ring wrap, the pair list, `first`,
    the staging area (lone-frame rule included), the lane in each form and the pending() sum equal the parent commit's."""
    out = _run(program)
    m = re.match(r"stream ledger ok: (\d+) sequences, (\d+) chunks, (\d+) lone frames, (\d+) failed chunks, (\d+) refused for room, "
                 r"(\d+) sequences with a dropped lone frame", out)
    assert m, out
    sequences, chunks, lone, failed, busy, drops = map(int, m.groups())
    assert sequences >= 20000 and min(chunks, lone, failed, busy, drops) > 1000, out   # every kind of step was really taken


def test_result_layout_equals_the_parent_commit(program):
    """Offsets and size for B in {1, 4, 5, 128, 1024} x cap in {1, 600, 2000, PS_MAX_KPTS}; the device and host views; the five
    segments of P in {1, B - 1, B} pairs against the three forms they replace (the 4-byte mask rounding of the copy kernel's)."""
    assert _run(program, "layout").strip() == "result layout ok"
