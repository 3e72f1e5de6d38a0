"""The CPU implementations of guided map matching -- oracle.match_xyz (binary rows) and tests/map_l2_ref.py::match_xyz_l2 (float
rows) -- held to the independent float64 model of tests/match_xyz_model_f64.py through its shared check; the ladder and the
predicted level against the model's; the directed scenes; and ten mutations of the model, each of which must fail the same check
against the unmodified implementations.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_l2_ref as lref  # noqa: E402
import map_pairs_ref as mref  # noqa: E402
import match_xyz_model_f64 as model  # noqa: E402

from putslam_amd import api, synth  # noqa: E402


def synth_kind(name):
    return (lambda g, n: synth.float_rows(g, n, name)), (lambda g, rows, src: synth.float_rows_linked(g, rows, src, name))


KINDS = {"binary": "binary", "surf": synth_kind("surf"), "sift": synth_kind("sift"), "w20": 20}


def implementation(oracle, kind):
    return oracle.match_xyz if kind == "binary" else lref.match_xyz_l2


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", model.SCENES, ids=lambda s: "%dx%d" % s)
def test_implementations_against_the_model(oracle, shape, kind):
    """Every scene at tries 1, 5 and 10 of the ladder: the emitted (queryIdx, trainIdx) sequence, imgIdx, the distance (binary:
    equal; float: within 4 u) and the cap on ambiguous features."""
    s = model.scene(np.random.default_rng(2000 + model.SCENES.index(shape)), *shape, KINDS[kind])
    for k in model.TRIES:
        r, a = model.ladder(model.RADIUS, model.RATIO, k)
        ans = model.match_xyz(*model.args(s), r, a)
        got = implementation(oracle, kind)(*model.args(s), r, a)
        rep = model.check(got, ans, (kind, shape, k))
        print("%s %s try %d: %d matches, %d / %d features ambiguous, worst distance %.2f u"
              % (kind, shape, k, len(got), rep.ambiguous, rep.with_candidates, rep.worst_u))
        assert len(got) >= min(shape) // 4
        if not rep.ambiguous:
            assert [(int(q), int(t)) for q, t in zip(got["queryIdx"], got["trainIdx"])] == ans.pairs()


def test_float32_norm_stays_inside_the_margin():
    """The model's own float32 norm against its float64 norm on all scenes: under 2.2e-7, a quarter of W."""
    worst, near, pairs = model.norm32_margin(model.SCENES)
    print("largest |d32 / d64 - 1| = %.3e over %d pairs; %d pairs within W of a ladder radius" % (worst, pairs, near))
    assert pairs == sum(a * b for a, b in model.SCENES)
    assert worst < model.NORM32_BOUND
    assert 4 * worst < model.W


def test_ladder():
    for k in range(1, 13):
        for r, a in ((0.12, 0.55), (0.05, 0.3), (1.0, 0.9), (0.12, 0.12)):
            want = model.ladder(r, a, k)
            assert api.ladder_try(r, a, k) == want, (k, r, a)
            assert mref.ladder_try(r, a, k) == want, (k, r, a)
    assert model.ladder(0.12, 0.55, 10) == (0.12 + 0.02 * 9, 0.55 - 0.05 * 9) and model.ladder(0.12, 0.55, 11) == (0.12 + 0.02 * 10, 0.1)
    assert model.ladder(0.12, 0.55, 1) == (0.12, 0.55) and model.ladder(0.12, 0.05, 1) == (0.12, 0.05)      # (try 1: as given)


def test_predicted_level(oracle):
    """10^5 random inputs that are not within 1e-9 of a switching point, and the clamps at both ends."""
    rng = np.random.default_rng(77)
    n = 100000
    octave = rng.integers(0, 8, n)
    cur = rng.uniform(0.3, 6.0, n)
    det = cur * 10 ** rng.uniform(-0.8, 0.8, n)
    level, amb = model.predicted_level(octave, det, cur)
    assert amb.sum() < 10 and set(level.tolist()) == set(range(8))
    assert (level == 0).sum() > 1000 and (level == 7).sum() > 1000
    got = np.array([oracle.predicted_level(int(o), float(d), float(c)) for o, d, c in zip(octave, det, cur)])
    assert np.array_equal(got[~amb], level[~amb])
    # exact powers: 1.2^o x 1 / 1 has quotient o up to rounding -- ambiguous by the model's rule, whatever a libm answers
    assert model.predicted_level(np.arange(8), np.ones(8), np.ones(8))[1].all()


@pytest.mark.parametrize("kind", list(KINDS))
def test_directed_scenes(oracle, kind):
    """15 / 16 / 17 candidates, candidates at keypoints 1023 and 1024 only, ratio x value == bestVal, a first candidate that is not
    the least (the scenes assert from the model's counts that they are what they are named)."""
    for name, s, r, a in model.directed(np.random.default_rng(31), KINDS[kind]):
        ans = model.match_xyz(*model.args(s), r, a)
        assert not ans.ambiguous and ans.exact, name
        got = implementation(oracle, kind)(*model.args(s), r, a)
        model.check(got, ans, (kind, name))
        assert [(int(m["queryIdx"]), int(m["trainIdx"])) for m in got] == ans.pairs(), name


def mutation_cases(kind):
    """[(name, scene, base radius, base ratio, try)]: two random scenes at tries 1, 5 and 10, and the directed scenes."""
    cases = []
    for n, shape in enumerate(model.SCENES[:2]):
        s = model.scene(np.random.default_rng(2000 + n), *shape, kind)
        cases += [("%dx%d" % shape, s, model.RADIUS, model.RATIO, k) for k in model.TRIES]
    cases += [(name, s, r, a, 1) for name, s, r, a in model.directed(np.random.default_rng(31), kind)]
    return cases


@pytest.fixture(scope="module")
def lists(oracle):
    """The unmodified implementations' match lists on the mutation cases, computed once."""
    out = {}
    for kind in ("binary", "surf"):
        cases = mutation_cases(KINDS[kind])
        out[kind] = [(c, implementation(oracle, kind)(*model.args(c[1]), *model.ladder(c[2], c[3], c[4]))) for c in cases]
    return out


# features flipped per mutation on mutation_cases (binary rows against oracle.match_xyz; no_sqrt: SURF rows against the
# restatement), as measured; the test asserts the measured figures so that a weaker scene set shows
FLIPPED = {"cur_minus_map": 105, "xor": 68, "window0": 485, "window2": 319, "strict_ratio": 1, "ratio_on_best": 780,
           "first_best": 112, "ladder_k": 87, "no_sqrt": 70, "best_only": 161}


@pytest.mark.parametrize("mutation", model.MUTATIONS)
def test_mutations_are_caught(lists, mutation):
    """Each other reading of matcher.cpp fails the shared check against the unmodified implementation on at least one scene."""
    kind = "surf" if mutation == "no_sqrt" else "binary"
    flipped, caught, off = 0, [], 0
    for (name, s, r0, a0, k), got in lists[kind]:
        r, a = model.ladder(r0, a0, k, mutation)
        rep = model.compare(got, model.match_xyz(*model.args(s), r, a, mutation))
        flipped += len(rep.flipped)
        off += rep.dist_bad
        if rep.failures():
            caught.append((name, k))
            with pytest.raises(AssertionError):
                model.check(got, model.match_xyz(*model.args(s), r, a, mutation))
    print("%s: %d features flipped, %d distances off, caught on %d of %d cases" % (mutation, flipped, off, len(caught), len(lists[kind])))
    assert caught and flipped + off > 0, mutation
    assert FLIPPED[mutation] == flipped, (mutation, flipped)
    # and the unmutated model passes on every one of these cases
    for (name, s, r0, a0, k), got in lists[kind]:
        model.check(got, model.match_xyz(*model.args(s), *model.ladder(r0, a0, k)), (kind, name, k))


@pytest.mark.parametrize("seed", [5, 1905])
def test_fuzz_map_draws_on_the_host(oracle, seed):
    """The configurations that tests/test_gpu_fuzz_slice.py::test_fuzz_map_slice draws, on the CPU: the oracle and the restatement
    pass the shared check on every pair, the cap on ambiguous features included (so the GPU slice's scenes stay inside it by the
    model alone), and the draws cover what the slice is for."""
    import fuzz_gpu
    rng = np.random.default_rng(seed)
    seen = dict(binary=0, float=0, pitched=0, per_pair=0, short=0, empty=0, outside=0, widths=set())
    for _ in range(20):
        cfg = fuzz_gpu.draw_map(rng)
        answers = fuzz_gpu.map_answers(cfg)
        assert not fuzz_gpu.map_model_failures(answers)
        cap = fuzz_gpu.map_max_matches(cfg, answers)
        V, F = len(cfg["views"]["nkpts"]), len(cfg["frames"]["nkpts"])
        seen["binary" if cfg["kind"] == "binary" else "float"] += 1
        seen["widths"].add(cfg["kind"])
        seen["pitched"] += cfg["pitched"]
        seen["per_pair"] += np.ndim(cfg["radius"]) > 0
        seen["short"] += any(len(m) > cap for m, _ in answers)
        seen["empty"] += int((cfg["views"]["nkpts"] == 0).any() or (cfg["frames"]["nkpts"] == 0).any())
        seen["outside"] += int(any(not (0 <= v < V and 0 <= f < F) for v, f in cfg["pairs"]))
        assert 1 <= len(cfg["pairs"]) <= 80 and max(cfg["views"]["cap"], cfg["frames"]["cap"]) <= 600
    print(seen)
    assert min(seen[k] for k in ("binary", "float", "pitched", "per_pair", "short", "empty", "outside")) >= 2, seen
    assert len(seen["widths"]) >= 4, seen
