"""The CPU oracle against the independent float64 model of tests/ransac_model_f64.py: per-hypothesis counts, selection, refit,
final mask and gate of RANSAC.cpp:50-174, on inputs whose errors lie on both sides of the thresholds, a camera with
fy = 0.8 fx and cx != cy, and with the model's own mutations to show that a wrong formula would be noticed.  No GPU.

The margin W and the Umeyama bounds are measured, not chosen: see the model file's docstring and UMEYAMA_BOUNDS."""
import os
import sys

import numpy as np
import pytest

from putslam_amd._abi import DMATCH_DTYPE, EST_FIXED, EST_RANSAC, default_ransac_params, make_config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_model_f64 as rm  # noqa: E402


def _matches(n):
    m = np.zeros(n, DMATCH_DTYPE)
    m["queryIdx"] = m["trainIdx"] = np.arange(n)
    return m


def _params(run):
    name, ci, n, mode, K, thrE, thrR, ds = run
    prm = default_ransac_params(mode)
    prm.inlierThresholdEuclidean, prm.inlierThresholdReprojection = thrE, thrR
    return prm


def _oracle_counts(oracle, run, raw=None):
    prev, cur, q, t, raw0 = rm.run_input(run)
    raw = raw0 if raw is None else raw
    cfg, keep = make_config(EST_FIXED, len(raw), sample_idx=raw)
    return oracle.hypothesis_counts(_params(run), cfg, run[4], prev, cur, _matches(len(q)))


def _oracle_call(oracle, run, est, raw=None):
    prev, cur, q, t, raw0 = rm.run_input(run)
    raw = raw0 if raw is None else raw
    cfg, keep = make_config(est, len(raw), sample_idx=raw)
    return oracle.ransac_rigid3d(_params(run), cfg, run[4], prev, cur, _matches(len(q)))


def _run(name):
    return next(r for r in rm.RUNS if r[0] == name)


# ------------------------------------------------------------------------------------------------ the model's own pieces
def test_model_depth_filter_and_sample_rule(oracle):
    prev, cur, q, t, raw = rm.run_input(_run("class0-mode0"))
    kept = rm.depth_filter(prev, cur, q, t)
    assert len(kept) == 254 and sorted(set(range(257)) - set(kept.tolist())) == [20, 70, 100]
    assert prev[130, 2] == np.float32(0.1) and prev[200, 2] == np.float32(6.0)          # the edges themselves stay
    # a repeat moves on to the next free index
    got = rm.sample_explicit(np.uint32([[7, 7, 7], [0, 1, 0], [1199, 1199, 0], [5, 6, 7]]), 1200)
    assert got.tolist() == [[7, 8, 9], [0, 1, 2], [1199, 0, 1], [5, 6, 7]]
    assert rm.sample_explicit(np.uint32([[2, 2, 2], [5, 4, 3]]), 3).tolist() == [[2, 0, 1], [2, 1, 0]]
    # the seeded stream (used by the batched GPU test only): the documented draw, a repeat drawn again
    for seed, M in ((1, 254), (2 ** 63 + 12345, 7), (77, 3)):
        cfg, _ = make_config(EST_FIXED, 64, seed=seed)
        assert int(rm.draw31(seed, 5, 2)) == oracle.draw31(seed, 5, 2)
        assert rm.sample_seeded(seed, 64, M).tolist() == [oracle.sample_triplet(cfg, h, M) for h in range(64)]


def test_float32_run_of_the_model_stays_inside_w():
    """The measurement behind W, repeated: the naive float32 run of the model needs at most W / 4 on every committed run."""
    worst = max(w for w, _ in rm.measure_w().values())
    print("measured w %.3g, W %.3g" % (worst, rm.W))
    assert 4 * worst <= rm.W <= 1e-2


# ------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("run", rm.RUNS, ids=[r[0] for r in rm.RUNS])
def test_oracle_counts_lie_in_the_models_brackets(oracle, run):
    counts, M = _oracle_counts(oracle, run)
    model = rm.run_model(run)
    bad, aside = rm.check_counts(model, counts, M)
    lo, hi = model.count_bracket() if model.M >= 3 else (np.zeros(1), np.zeros(1))
    print("%s: M %d, set aside %d of %d, brackets open on %d" % (run[0], M, aside, model.H, int((lo != hi).sum())))
    assert not bad, bad[:5]
    if model.M > 3:       # (M = 3: every hypothesis is the same triangle, well conditioned or not)
        assert aside <= rm.COND_CAP * model.H, aside


def test_dead_and_unknown_modes_count_nothing(oracle):
    """Mahalanobis (RANSAC.cpp:301-303: the covariance is never filled) and an unknown error version (:134-135)."""
    base = _run("class1-mode0")
    for mode in (rm.MAHALANOBIS, 7):
        run = base[:3] + (mode,) + base[4:]
        counts, M = _oracle_counts(oracle, run)
        model = rm.run_model(run, mutation=None, raw=rm.run_input(run)[4])
        assert M == model.M == 254 and not counts.any() and not model.counts().any()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("est", [EST_FIXED, EST_RANSAC])
def test_oracle_end_to_end_against_the_model(oracle, est):
    open_cases = 0
    for run in rm.RUNS:
        res = _oracle_call(oracle, run, est)
        bad, selection_only = rm.check_end_to_end(rm.run_model(run), res, est == EST_FIXED)
        st = res["stats"]
        print("%s: best %d count %d its %d inliers %d accepted %d%s" % (
            run[0], st["bestHypothesis"], st["bestInlierCount"], st["iterationsRun"], st["numInliers"], st["accepted"],
            "  (selection only)" if selection_only else ""))
        assert not bad, (run[0], bad[:5])
        open_cases += selection_only
    assert 10 * open_cases <= len(rm.RUNS), open_cases


def test_model_run_agrees_with_the_oracle_where_it_is_determined(oracle):
    """Model.run -- the model's own answer, no brackets -- on the cases whose best bracket is empty: same hypothesis, count,
    ratio bits, gate; the mask apart from matches within W of the final threshold."""
    for run in rm.RUNS:
        model = rm.run_model(run)
        res = _oracle_call(oracle, run, EST_FIXED)
        st, own = res["stats"], model.run(model.H)
        if own["best"] < 0:
            assert st["bestHypothesis"] == -1 and st["accepted"] == 0
            continue
        lo, hi = model.count_bracket()
        if (lo != hi)[: model.H].any():        # some bracket open: the arg-max itself may differ
            continue
        assert own["best"] == st["bestHypothesis"] and own["count"] == st["bestInlierCount"]
        assert own["ratio"].tobytes() == np.float32(st["bestInlierRatio"]).tobytes() and own["accepted"] == st["accepted"]
        if own["accepted"]:
            assert np.abs(res["pose"] - own["pose"]).max() < rm.REFIT_TOL
            assert abs(int(st["numInliers"]) - own["numInliers"]) <= 2


# ------------------------------------------------------------------------------------------------ teeth
COUNT_TEETH = [("adaptive_cur_z", "class0-mode4"),
               ("one_direction", "class0-mode1"), ("one_direction", "class0-mode2"),
               ("real_new_from_prev", "class0-mode1"), ("real_new_from_prev", "class0-mode2"),
               ("no_inverse", "class0-mode1"), ("no_inverse", "class0-mode2"),
               ("fx_for_v", "class0-mode1"), ("fx_for_v", "class0-mode2")]


@pytest.mark.parametrize("mutation,name", COUNT_TEETH)
def test_a_mutated_model_does_not_hold_the_oracles_counts(oracle, mutation, name):
    run = _run(name)
    counts, M = _oracle_counts(oracle, run)
    bad, _ = rm.check_counts(rm.run_model(run, mutation=mutation), counts, M)
    print("%s on %s: caught on %d of %d hypotheses" % (mutation, name, len(bad), len(counts)))
    assert len(bad) >= 5, len(bad)


def test_a_model_that_reselects_with_the_loops_metric_is_caught(oracle):
    caught = 0
    for name in ("class1-mode1", "halved-mode1"):       # (accepted calls: a rejected one has no final mask to tell by)
        run = _run(name)
        res = _oracle_call(oracle, run, EST_FIXED)
        good, only = rm.check_end_to_end(rm.run_model(run), res, True)
        bad, _ = rm.check_end_to_end(rm.run_model(run, mutation="refit_reprojection"), res, True)
        print("refit_reprojection on %s: %s" % (name, bad))
        assert not good
        caught += bool(bad) and not only
    print("refit_reprojection: caught on %d of 2 runs" % caught)
    assert caught == 2


def test_a_model_that_takes_the_last_maximum_is_caught(oracle):
    """Two hypotheses drawn from the same triplet: the best one's draws are repeated in the last hypothesis."""
    caught = 0
    for name in ("class0-mode0", "class1-mode1", "class0-mode4"):
        run = _run(name)
        model = rm.run_model(run)
        raw = rm.run_input(run)[4].copy()
        b = model.select(model.H)
        raw[-1] = raw[b]
        res = _oracle_call(oracle, run, EST_FIXED, raw)
        assert res["stats"]["bestHypothesis"] == b
        good, _ = rm.check_end_to_end(rm.run_model(run, raw=raw), res, True)
        bad, _ = rm.check_end_to_end(rm.run_model(run, raw=raw, mutation="last_max"), res, True)
        print("last_max on %s: %s" % (name, bad))
        assert not good
        caught += bool(bad)
    print("last_max: caught on %d of 3 runs" % caught)
    assert caught == 3


# ------------------------------------------------------------------------------------------------ the refit on its own
@pytest.mark.parametrize("family", rm.FAMILIES)
def test_oracle_umeyama_against_the_long_double_fit(oracle, family):
    for k in rm.UMEYAMA_K:
        src, dst = rm.umeyama_sets(family, k)
        T = np.stack([oracle.umeyama_f32(src[i], dst[i])[0] for i in range(len(src))])
        bad, worst = rm.check_umeyama(family, k, src, dst, T)
        print("%s k=%d: det %.2g orth %.2g excess %.3g pose %.3g" % ((family, k) + tuple(worst)))
        assert not bad, bad[:5]
