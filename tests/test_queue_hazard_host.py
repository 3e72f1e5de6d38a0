"""PsBatchQueue's hazard rule (putslam_amd/csrc/ps_queue_hazard.h: which chain a batch runs on and which events that chain waits
for first, given the tickets still in the ring) compiled into a plain C++ program -- no HIP header, no GPU -- and run:
tests/cpp/test_queue_hazard.cpp walks every sequence of submits and completions and holds the checker.  Then the bookkeeping the
queue had before, as a Python model (tests/queue_hazard_model.py): the safety check rejects it, first at the sequences of the table."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import queue_hazard_model as M  # noqa: E402


def test_queue_hazard_program(tmp_path):
    exe = str(tmp_path / "test_queue_hazard")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "putslam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_queue_hazard.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "queue hazard ok", run.stdout


# chains -> the shortest submit sequence that made a batch run beside its predecessors, and on which chains
TABLE = {2: ("AABA", [0, 0, 0, 1], [0, 1]), 3: ("AAABA", [0, 0, 0, 0, 1], [0, 1, 2]), 4: ("AAAABA", [0, 0, 0, 0, 0, 1], [0, 1, 2, 3])}


@pytest.mark.parametrize("chains", [2, 3, 4])
def test_the_old_rule_is_rejected_at_the_tabled_sequences(chains):
    """Submits and completions over two blocks: nothing shorter than the table's sequence is rejected, and at its length that
    sequence alone -- with no completion in it, only batches still in flight.  A third block adds ways to make a chain forget
    (A B C A at two chains: C lands on chain 0 and A is forgotten there) but nothing shorter and nothing that needs a completion.
    The batch that breaks the rule runs on chain 1 against all the block-A batches in flight on chain 0."""
    ops, chain_of, beside = TABLE[chains]
    two, three = M.rejected_sequences(chains, len(ops), blocks=2), M.rejected_sequences(chains, len(ops), blocks=3)
    for length in range(1, len(ops)):
        assert two[length] == [] and three[length] == []
    assert two[len(ops)] == [ops]
    assert three[len(ops)][0] == ops and all(s.isalpha() and s[-1] == "A" and "C" in s for s in three[len(ops)][1:])
    at, bad, chains_seen = M.run(chains, ops)
    assert at == len(ops) - 1 and bad == beside and chains_seen == chain_of


def test_the_old_rule_fails_the_rotation_once_some_batches_are_complete():
    """Three blocks on four chains with batches completing in between (the advisor's scenario): B in flight on chain 1, C is
    redirected there, the next B runs on another chain."""
    ops = "ABC" + "2" + "AA"      # A -> 0, B -> 1, C -> 2; C completes; two more on A follow their predecessor on chain 0
    at, _, chain_of = M.run(4, ops)
    assert at is None and chain_of == [0, 1, 2, 0, 0]
    ops += "C" + "B"              # batch 5: C, nothing of it in flight, on its nominal chain 1 -- which forgets B; batch 6: B, nominal 2
    at, bad, chain_of = M.run(4, ops)
    assert chain_of[5] == 1 and chain_of[6] == 2          # ... beside batch 1, B, still in flight on chain 1
    assert at == len(ops) - 1 and bad == [1]


def test_the_model_holds_where_the_old_rule_was_right():
    """One block on two chains, the case the suite had: every batch follows its predecessor while it is in flight."""
    at, _, chain_of = M.run(2, "AAAAAA")
    assert at is None and chain_of == [0] * 6
    at, _, chain_of = M.run(2, "A0A1A")                   # complete predecessors: the chains in turn
    assert at is None and chain_of == [0, 1, 0]
    assert M.canonical("CCAC") == "AABA"
