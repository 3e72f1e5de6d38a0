"""What the slices of tests/test_gpu_fuzz_front_end_slice.py reach, shown on the restatements alone: the draws of
tests/fuzz_front_end.py (SLICE_SEEDS x SLICE_DRAWS, the very draws the GPU tests make) run through klt_ref, fast_ref,
orb_detect_ref, orb_ref and track_close_ref, and the conditions a slice must meet to be worth its GPU time asserted on the
results -- every exit of the tracker, every class of window against the wave width, lists that are cut, key points that are kept
and dropped, samples outside their level, every tile seam of the merge.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import fast_ref as F  # noqa: E402
import fuzz_front_end as Z  # noqa: E402
import klt_ref as K  # noqa: E402

SEEDS = Z.SLICE_SEEDS


def test_the_slices_are_what_the_issue_starts_from():
    assert Z.SLICE_SEEDS == (11, 2026) and Z.SLICE_DRAWS == dict(klt=24, fast=40, orb_detect=40, orb_describe=40, merge=40)
    for family in Z.FAMILIES:     # a draw is plain data and the same every time
        a, b = Z.slice_draws(family, 3, 4), Z.slice_draws(family, 3, 4)
        assert repr(a) == repr(b) and all(isinstance(d, dict) and "redraws" in d for d in a)


def test_the_klt_classes_cover_every_legal_window():
    wins = {(w, cn) for w in range(3, 32) for cn in (1, 3)}
    assert set().union(*[set(v) for v in Z.KLT_CLASSES.values()]) == wins
    for name, members in Z.KLT_CLASSES.items():
        assert all(Z.klt_class(w, cn) == name for w, cn in members)
    assert Z.klt_class(21, 3) == "below" and Z.klt_class(22, 3) == "above" and 64 % 63 == 1 and 64 // 66 == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_klt_slice(seed):
    draws = Z.slice_draws("klt", seed)
    exits, mixed = {}, 0
    for cfg in draws:
        want = Z.klt_reference(cfg, exits=exits)
        status = np.concatenate([w[1] for w in want])
        mixed += bool(status.any() and not status.all())
    print("klt", seed, exits, "mixed", mixed)
    assert all(exits[k] > 0 for k in K.EXITS), exits
    assert 2 * mixed >= len(draws)
    assert {d["cols"] % 4 for d in draws} == {0, 1, 2, 3}
    assert {d["cls"] for d in draws} == {"divides", "below", "above"} and all(d["cls"] == Z.klt_class(d["win"], d["cn"]) for d in draws)
    assert {63, 66} <= {d["win"] * d["cn"] for d in draws}
    built = [(K.level_count(d["rows"], d["cols"], d["win"], d["max_levels"]), d["max_levels"]) for d in draws]
    assert sum(L < m for L, m in built) >= 2 and sum(L == m and m > 0 for L, m in built) >= 2, built


@pytest.mark.parametrize("seed", SEEDS)
def test_fast_slice(seed):
    draws = Z.slice_draws("fast", seed)
    emit = cut = 0
    for cfg in draws:
        imgs = Z.fast_inputs(cfg)
        got = [len(w[1][1]) for w in Z.fast_reference(cfg, imgs)]
        emit += any(got)
        if any(got):
            free = [len(w[1][1]) for w in Z.fast_reference(cfg, imgs, max_features=10 ** 6)]
            cut += any(f > g > 0 for f, g in zip(free, got))
    print("fast", seed, "emit", emit, "cut", cut)
    assert len(draws) == 40 and emit >= 16 and cut >= 10
    assert {d["cols"] % 4 for d in draws} == {0, 1, 2, 3}


@pytest.mark.parametrize("seed", SEEDS)
def test_orb_detect_slice(seed):
    draws = Z.slice_draws("orb_detect", seed)
    keep = drop = 0
    for cfg in draws:
        assert Z.orb_detect_premise(cfg)
        t = F.clamp_threshold(cfg["fast_threshold"])
        kept_any = dropped = False
        for xy, _, _, _, rois in Z.orb_detect_reference(cfg):
            kept_any |= len(xy) > 0
            survivors = 0
            for levels in rois:
                for lv in levels:
                    emitted = int(F.emitted_closed(*F.fast_closed(lv["raw"], t), True)[0].sum())
                    dropped |= emitted > int(lv["kept"].sum())          # the border, or one of the two quotas
                    survivors += int(lv["kept"].sum())
            dropped |= survivors > len(xy)                              # the cut per ROI, or the maximum
        keep, drop = keep + kept_any, drop + dropped
    redraws = sum(d["redraws"] for d in draws)
    print("orb_detect", seed, "keep", keep, "drop", drop, "redraws", redraws)
    assert 2 * keep >= len(draws) and 4 * drop >= len(draws) and 10 * redraws <= len(draws)


@pytest.mark.parametrize("seed", SEEDS)
def test_orb_describe_slice(seed):
    draws = Z.slice_draws("orb_describe", seed)
    keep = drop = outside = 0
    for cfg in draws:
        _, want, cnt = Z.orb_describe_reference(cfg)
        assert cnt["reach"] <= Z.REACH_MAX
        keep += any(len(k) > 0 for _, k in want)
        drop += any(len(k) < c for (_, k), c in zip(want, cfg["counts"]))
        outside += cnt["outside"] > 0
    redraws = sum(d["redraws"] for d in draws)
    print("orb_describe", seed, "keep", keep, "drop", drop, "outside", outside, "redraws", redraws)
    assert 2 * keep >= len(draws) and 4 * drop >= len(draws) and 4 * outside >= len(draws) and 10 * redraws <= len(draws)
    assert {(d["rows"], d["cols"]) for d in draws} != {(80, 96)} and len({(d["rows"], d["cols"]) for d in draws}) > 30


@pytest.mark.parametrize("seed", SEEDS)
def test_merge_slice(seed):
    draws = Z.slice_draws("merge", seed)
    tracked, cands, refill, before_last, only_earlier, second_trip = set(), set(), set(), 0, 0, 0
    for cfg in draws:
        inputs = Z.merge_inputs(cfg)
        want = Z.merge_reference(cfg, inputs)
        assert Z.merge_premise(want)
        tracked |= set(cfg["tracked"])
        cands |= {c for c in cfg["candidates"] if c >= 0}
        refill |= {w["refill"] for w in want}
        seams = [Z.merge_seams(t, c, w, cfg["min_dist"]) for (t, c), w in zip(inputs, want)]
        before_last += any(a > Z.TILE for a, _, _ in seams)
        only_earlier += any(len(r) > 0 for _, r, _ in seams)
        second_trip += any(len(r) > 0 for _, _, r in seams)
    print("merge", seed, "more than a tile accepted before the last tile:", before_last, "rejected by an earlier tile only:", only_earlier,
          "rejected by the second trip over the accepted candidates only:", second_trip, "redraws", sum(d["redraws"] for d in draws))
    assert tracked == set(Z.TRACKED_COUNTS) and cands == set(Z.CANDIDATE_COUNTS) and refill == {0, 1, 2}
    assert before_last >= 1 and only_earlier >= 1
    assert second_trip >= 1      # (a sweep of the accepted candidates that stops at 256 gives another answer in this slice)
    assert 10 * sum(d["redraws"] for d in draws) <= len(draws)
