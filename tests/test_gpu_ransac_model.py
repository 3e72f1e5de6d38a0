"""The scoring, selection and refit kernels (ps_ransac_score<KIND>, ps_ransac_score_fast, ps_ransac_score_euclid,
ps_select_refit, wave_umeyama) against the independent float64 model of tests/ransac_model_f64.py -- directly: the oracle is
not used here.  Inputs and checks are those of tests/test_ransac_model_host.py (same runs, same brackets at the measured
margin W, same conditioning cap, same 1-in-10 cap on cases checked up to the selection only).

ps_umeyama_f32 on its own is held to the long-double fit over eight families x k = 3, 4, 64, 65, 1000 x 200 sets
(rm.umeyama_sets): |det R - 1| and |R R^T - I| below 1e-5; the mean squared residual within 4 x the bound of the table
below of the optimum; for the families whose data determines the rotation (all but collinear and thin) the pose within
4 x the table's.  The table is what numpy's float32 SVD fit (rm.numpy_f32_fit: the same formulas, LAPACK's SVD, nothing of
the project's) reaches on the same sets, measured on a CPU by rm.measure_umeyama():

  worst residual excess in units of eps32 sigma_src sigma_dst  /  worst pose difference (rotation entries; translation
  relative to 1 + the larger centroid norm), before the floor of 16 (excess) and 16 eps32 = 1.9e-6 (pose):

                 k = 3              k = 4              k = 64             k = 65             k = 1000
    good         0.015 / 5e-07      0.0037 / 2.7e-07   0.0012 / 3.3e-07   0.00083 / 3.8e-07  0.00032 / 1.2e-06
    far          0.012 / 4.3e-07    0.0029 / 2.4e-07   0.0062 / 3e-07     0.0066 / 3.1e-07   0.086 / 1.1e-06
    planar       0.016 / 3.2e-07    0.0079 / 2.3e-07   0.0015 / 2.6e-07   0.0014 / 2.3e-07   0.00041 / 1.1e-06
    near_planar  0.015 / 1.7e-07    0.009 / 1.2e-07    0.0015 / 3.3e-07   0.0012 / 3.8e-07   0.00051 / 1.5e-06
    collinear    0.015 / -          0.0087 / -         0.0011 / -         0.0011 / -         0.00042 / -
    thin         0.065 / -          0.025 / -          0.0021 / -         0.0022 / -         0.00069 / -
    tiny         0.0073 / 2.7e-07   0.0084 / 4.9e-07   0.00073 / 1.3e-07  0.00077 / 1.7e-07  0.00045 / 3.5e-07
    huge         0.0052 / 3.3e-07   0.0048 / 2.4e-07   0.00087 / 6.2e-07  0.0012 / 5.3e-07   0.00041 / 1.9e-06

  Every figure lies under its floor (the excess is of second order in the pose's error), so rm.UMEYAMA_BOUNDS holds the
  floors and the kernels are allowed 64 eps32 sigma_src sigma_dst of residual and 7.6e-6 of pose.  A family whose pose is
  asserted holds no slim set (sigma_1 <= 20 (sigma_2 + sigma_3), rm.KAPPA_MAX): without that rule the worst of 200 random
  triangles decides the figure (6.5e-5 for numpy, 2.6e-4 for the restated Jacobi SVD on near_planar k = 3), which says
  how slim the slimmest triangle was and nothing about the fit.
"""
import os
import sys

import numpy as np
import pytest

from putslam_amd import api
from putslam_amd._abi import DMATCH_DTYPE, EST_FIXED, EST_RANSAC, default_ransac_params, make_config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_model_f64 as rm  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fctx():
    c = api.Context(0)
    c.set_option("score", 1)            # the decision-exact kernels (the default)
    c.set_option("score_stats", 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ectx():
    c = api.Context(0)
    c.set_option("score", 0)            # the value-exact kernel
    yield c
    c.close()


def _matches(n):
    m = np.zeros(n, DMATCH_DTYPE)
    m["queryIdx"] = m["trainIdx"] = np.arange(n)
    return m


def _params(run):
    name, ci, n, mode, K, thrE, thrR, ds = run
    prm = default_ransac_params(mode)
    prm.inlierThresholdEuclidean, prm.inlierThresholdReprojection = thrE, thrR
    return prm


def _run(name):
    return next(r for r in rm.RUNS if r[0] == name)


def _counts(ctx, run, raw=None):
    prev, cur, q, t, raw0 = rm.run_input(run)
    raw = raw0 if raw is None else raw
    cfg, keep = make_config(EST_FIXED, len(raw), sample_idx=raw)
    prm = _params(run)
    prm.minimalNumberOfMatches = 3      # (the diagnostic is the call's scoring stage: below the minimum it scores nothing)
    return ctx.debug_ransac_counts(prm, cfg, run[4], prev, cur, _matches(len(q)))


def _call(ctx, run, est, raw=None):
    prev, cur, q, t, raw0 = rm.run_input(run)
    raw = raw0 if raw is None else raw
    cfg, keep = make_config(est, len(raw), sample_idx=raw)
    return ctx.ransac_rigid3d(_params(run), cfg, run[4], prev, cur, _matches(len(q)))


# ------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("run", rm.RUNS, ids=[r[0] for r in rm.RUNS])
def test_kernel_counts_lie_in_the_models_brackets(fctx, ectx, run):
    model = rm.run_model(run)
    for which, ctx in (("decision-exact", fctx), ("value-exact", ectx)):
        counts = _counts(ctx, run)
        assert len(counts) == model.H
        bad, aside = rm.check_counts(model, counts, model.M)
        print("%s %s: M %d, set aside %d of %d" % (run[0], which, model.M, aside, model.H))
        assert not bad, (which, bad[:5])
        if model.M > 3:
            assert aside <= rm.COND_CAP * model.H, aside
        if ctx is fctx:
            parked, evals = fctx.score_stats()
            print("%s: parked %d of %d evaluations" % (run[0], parked, evals))
            assert parked <= evals
            if model.M >= 3 and run[4] is not rm.K_SMALL:
                assert evals >= model.H * model.M, "the fast form did not run"


# ------------------------------------------------------------------------------------------------ ps_ransac_rigid3d
@pytest.mark.parametrize("est", [EST_FIXED, EST_RANSAC])
@pytest.mark.parametrize("score", [1, 0])
def test_kernels_end_to_end_against_the_model(fctx, ectx, score, est):
    ctx = fctx if score else ectx
    open_cases = 0
    for run in rm.RUNS:
        res = _call(ctx, run, est)
        bad, selection_only = rm.check_end_to_end(rm.run_model(run), res, est == EST_FIXED)
        st = res["stats"]
        print("%s: best %d count %d its %d inliers %d accepted %d%s" % (
            run[0], st["bestHypothesis"], st["bestInlierCount"], st["iterationsRun"], st["numInliers"], st["accepted"],
            "  (selection only)" if selection_only else ""))
        assert not bad, (run[0], bad[:5])
        open_cases += selection_only
    assert 10 * open_cases <= len(rm.RUNS), open_cases


# ------------------------------------------------------------------------------------------------ teeth
COUNT_TEETH = [("adaptive_cur_z", "class0-mode4"),
               ("one_direction", "class0-mode1"), ("one_direction", "class0-mode2"),
               ("real_new_from_prev", "class0-mode1"), ("real_new_from_prev", "class0-mode2"),
               ("no_inverse", "class0-mode1"), ("no_inverse", "class0-mode2"),
               ("fx_for_v", "class0-mode1"), ("fx_for_v", "class0-mode2")]


@pytest.mark.parametrize("mutation,name", COUNT_TEETH)
def test_a_mutated_model_does_not_hold_the_kernels_counts(fctx, mutation, name):
    run = _run(name)
    counts = _counts(fctx, run)
    model = rm.run_model(run, mutation=mutation)
    bad, _ = rm.check_counts(model, counts, model.M)
    print("%s on %s: caught on %d of %d hypotheses" % (mutation, name, len(bad), len(counts)))
    assert len(bad) >= 5, len(bad)


def test_a_model_that_reselects_with_the_loops_metric_is_caught(fctx):
    caught = 0
    for name in ("class1-mode1", "halved-mode1"):       # (accepted calls: a rejected one has no final mask to tell by)
        run = _run(name)
        res = _call(fctx, run, EST_FIXED)
        good, only = rm.check_end_to_end(rm.run_model(run), res, True)
        bad, _ = rm.check_end_to_end(rm.run_model(run, mutation="refit_reprojection"), res, True)
        print("refit_reprojection on %s: %s" % (name, bad))
        assert not good
        caught += bool(bad) and not only
    print("refit_reprojection: caught on %d of 2 runs" % caught)
    assert caught == 2


def test_a_model_that_takes_the_last_maximum_is_caught(fctx):
    """Two hypotheses drawn from the same triplet: the best one's draws are repeated in the last hypothesis."""
    caught = 0
    for name in ("class0-mode0", "class1-mode1", "class0-mode4"):
        run = _run(name)
        model = rm.run_model(run)
        raw = rm.run_input(run)[4].copy()
        b = model.select(model.H)
        raw[-1] = raw[b]
        res = _call(fctx, run, EST_FIXED, raw)
        good, _ = rm.check_end_to_end(rm.run_model(run, raw=raw), res, True)
        bad, _ = rm.check_end_to_end(rm.run_model(run, raw=raw, mutation="last_max"), res, True)
        print("last_max on %s: %s" % (name, bad))
        assert not good
        caught += bool(bad)
    print("last_max: caught on %d of 3 runs" % caught)
    assert caught == 3


# ------------------------------------------------------------------------------------------------ one batch of 8 pairs
BATCH_H, BATCH_SEED = 1024, 4242


@pytest.fixture(scope="module")
def batch():
    """16 frames of 257 keypoints: frames 2p / 2p + 1 are pair p's previous / current frame and carry the same 257 distinct
    descriptors, so that the cross-check matcher returns the identity list."""
    rng = np.random.default_rng(31)
    P, n = 8, rm.N_FULL
    desc, pts = np.zeros((2 * P, n, 32), np.uint8), np.zeros((2 * P, n, 3), np.float32)
    for p in range(P):
        d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        assert len({bytes(r) for r in d}) == n
        desc[2 * p] = desc[2 * p + 1] = d
        pts[2 * p], pts[2 * p + 1], _, _ = rm.make_input(rm.CLASSES[p % 3], n, seed=100 + p)
    pairs = np.stack([np.arange(P) * 2, np.arange(P) * 2 + 1], 1).astype(np.int32)
    return dict(desc=desc, pts=pts, nkpts=np.full(2 * P, n, np.int32), pairs=pairs, models={})


def test_batch_of_pairs_staged_and_complete_against_the_model(batch):
    """ps_vo_pairs_device (matcher, scoring, selection, refit in one call) with the staged scoring forced on and forced off,
    in all four modes: 32 (mode, pair) cases, each in both forms."""
    open_cases = set()
    for mode in rm.MODES:
        _batch_mode(batch, mode, open_cases)
    assert 10 * len(open_cases) <= len(rm.MODES) * len(batch["pairs"]), sorted(open_cases)


def _batch_mode(batch, mode, open_cases):
    from putslam_amd.device_batch import FrameSetDevice, PairBatchDevice, run_pairs
    P, n = len(batch["pairs"]), rm.N_FULL
    prm = default_ransac_params(mode)
    cfg, _ = make_config(EST_FIXED, BATCH_H, seed=BATCH_SEED)
    ident = np.arange(n)
    for prune in (2, 0):                                   # staged scoring forced on / off (tests/test_gpu_prune.py's options)
        c = api.Context(0)
        c.set_option("prune", prune)
        c.set_option("reorder", 1)
        fs = FrameSetDevice(batch["desc"], batch["pts"], batch["nkpts"])
        pb = PairBatchDevice(batch["pairs"], fs.max_kpts)
        run_pairs(c, prm, cfg, rm.K_SKEW, fs, pb)
        g = pb.download()
        staged = c.get_option("last_staged_pairs")
        c.close()
        assert (staged > 0) == (prune == 2), staged
        for p in range(P):
            assert int(g["numMatches"][p]) == n
            assert np.array_equal(g["matches"][p, :n]["queryIdx"], ident) and np.array_equal(g["matches"][p, :n]["trainIdx"], ident)
            # pair p draws from seed + p
            model = rm.Model(batch["pts"][2 * p], batch["pts"][2 * p + 1], ident, ident, rm.K_SKEW, mode,
                             seed=BATCH_SEED + p, H=BATCH_H) if (mode, p) not in batch["models"] else batch["models"][mode, p]
            batch["models"][mode, p] = model
            res = dict(pose=g["pose"][p].reshape(4, 4).T, mask=g["inlierMask"][p, :n], stats=g["stats"][p])
            bad, selection_only = rm.check_end_to_end(model, res, True)
            print("mode %d prune %d pair %d: best %d count %d inliers %d accepted %d%s" % (
                mode, prune, p, res["stats"]["bestHypothesis"], res["stats"]["bestInlierCount"], res["stats"]["numInliers"],
                res["stats"]["accepted"], "  (selection only)" if selection_only else ""))
            assert not bad, (mode, prune, p, bad[:5])
            if selection_only:
                open_cases.add((mode, p))


# ------------------------------------------------------------------------------------------------ wave_umeyama on its own
@pytest.mark.parametrize("family", rm.FAMILIES)
def test_umeyama_kernel_against_the_long_double_fit(ctx, family):
    for k in rm.UMEYAMA_K:
        src, dst = rm.umeyama_sets(family, k)
        T, valid = ctx.umeyama_f32(src, dst)
        assert valid.all()
        bad, worst = rm.check_umeyama(family, k, src, dst, T)
        print("%s k=%d: det %.2g orth %.2g excess %.3g pose %.3g" % ((family, k) + tuple(worst)))
        assert not bad, bad[:5]
