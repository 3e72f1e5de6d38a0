"""The final drain of the decision-exact reprojection kernels (ps_score_fast.h): ONE per work-group.

A wave parks the evaluations its cheap value cannot decide in a queue of its own and, when the queue is full in the middle
of the sweep, evaluates them itself.  What is left at the END of the sweep is pooled: after a barrier the work-group takes the
four queues as one list, entry e to thread e in strides of 256, whichever wave parked it -- the waves without a hypothesis
and the ones that took the value-exact loop included.  These tests run the shapes where that can go wrong, small:
  * H = 64 and 300 leave waves without a hypothesis (one of four, and the ragged last block), H = 256 / 1024 fill them;
  * an odd number of matches parks all 64 lanes of every wave at its last match, so 64 / 256 entries per work-group are
    forced, and DUP copies of a match placed exactly on the decision boundary of one hypothesis (the trick of
    test_gpu_band_edges.py) put the list past 64 and past 256 entries: more than one stride;
  * errorVersion 1 and 2, fixed and adaptive schedules, complete (prune = 0) and staged (prune = 2: the looping stage 1 and
    the list stages with their split match ranges), one and two pairs, thresholds at the data's noise level.
Required: every hypothesis's count and every output equal the oracle's, and ps_debug_score_stats reports at least the
entries the shape forces (entries parked, not passes run)."""
import numpy as np
import pytest

from putslam_amd import api, synth
from putslam_amd._abi import (DMATCH_DTYPE, EST_FIXED, EST_RANSAC, EUCLIDEAN_AND_REPROJECTION_ERROR, REPROJECTION_ERROR, TUM_FR1_K,
                              default_ransac_params, make_config)

pytestmark = pytest.mark.gpu

NOISE = 0.004       # metres on every coordinate of the true correspondences: 0.7 px at 3 m, the thresholds below sit on it
STAT_FIELDS = ("numMatchesIn", "numMatchesValid", "bestHypothesis", "bestInlierCount", "iterationsRun", "numInliers",
               "accepted", "bestInlierRatio", "pointInlierRatio")


def _ctx(**options):
    c = api.Context(0)
    c.set_option("score", 1)
    c.set_option("score_stats", 1)
    for name, value in options.items():
        c.set_option(name, value)
    return c


def _scene(rng, n):
    prev = (rng.uniform(-1.5, 1.5, (n, 3)) + [0, 0, 3.2]).astype(np.float32)
    R, t = synth.random_motion(rng, 4.0, 0.08)
    cur = ((prev.astype(np.float64) - t) @ R + rng.normal(0, NOISE, (n, 3))).astype(np.float32)
    cur[:, 2] = np.clip(cur[:, 2], 0.2, 5.8)
    bad = rng.random(n) < 0.3
    cur[bad] = (rng.uniform(-1.5, 1.5, (int(bad.sum()), 3)) + [0, 0, 3.2]).astype(np.float32)
    return prev, cur


def _identity_matches(order):
    m = np.zeros(len(order), DMATCH_DTYPE)
    m["queryIdx"] = order
    m["trainIdx"] = order
    return m


def _noise_level_params(mode):
    prm = default_ransac_params(mode)
    prm.minimalNumberOfMatches = 3
    prm.inlierThresholdReprojection = 1.0            # pixels: the noise is 0.7 px at the scene's depth
    prm.inlierThresholdEuclidean = 0.007 if mode == EUCLIDEAN_AND_REPROJECTION_ERROR else 1e5   # sqrt(3) x NOISE
    return prm


# ---- every hypothesis's count, complete scoring of one pair ---------------------------------------------------------------
# (H, M): M odd -> the last match parks 64 entries in every wave that has a hypothesis
COUNT_SHAPES = [(64, 65), (256, 129), (300, 299), (1024, 201)]


@pytest.mark.parametrize("H,M", COUNT_SHAPES)
@pytest.mark.parametrize("est", [EST_FIXED, EST_RANSAC])
@pytest.mark.parametrize("mode", [REPROJECTION_ERROR, EUCLIDEAN_AND_REPROJECTION_ERROR])
def test_counts_with_an_odd_last_match(oracle, mode, est, H, M):
    ctx = _ctx()
    rng = np.random.default_rng(31 * H + M + 7 * mode + est)
    prev, cur = _scene(rng, M)
    m = _identity_matches(np.arange(M))
    prm = _noise_level_params(mode)
    cfg, _ = make_config(est, H, seed=H + M)
    got = ctx.debug_ransac_counts(prm, cfg, TUM_FR1_K, prev, cur, m)
    parked, evals = ctx.score_stats()
    want, Mv = oracle.hypothesis_counts(prm, cfg, TUM_FR1_K, prev, cur, m)
    print("mode %d est %d H %d M %d: scored %d, parked %d, evaluations %d" % (mode, est, H, M, len(got), parked, evals))
    assert Mv == M and len(got) > 0
    assert np.array_equal(got, want[: len(got)])
    assert evals >= len(got) * M, "the decision-exact path did not run"
    assert parked >= 64 * ((len(got) + 63) // 64), "the odd last match parks 64 lanes of every wave with a hypothesis"
    ctx.close()


# ---- more than one stride of entries in ONE final drain -------------------------------------------------------------------
def _boundary(oracle, mode, T, K, pp, cp, e):
    """Neighbouring doubles (t0, t1): the reference's reprojection test of this evaluation fails at t0 and passes at t1."""
    def passes(thr):
        return bool(oracle.is_inlier(mode, T, K, pp, cp, 1e5, thr))
    t = float(e)
    for _ in range(64):
        if passes(t):
            break
        t = np.nextafter(t, np.inf)
    assert passes(t)
    for _ in range(64):
        lower = np.nextafter(t, -np.inf)
        if not passes(lower):
            return lower, t
        t = lower
    raise AssertionError("no boundary found")


DUP = 26      # copies of the boundary match: 149 other matches + 26 = 175, odd


@pytest.mark.parametrize("H", [64, 256])
def test_final_drain_longer_than_one_stride(oracle, H):
    """One work-group sweeps all matches of H hypotheses (match range not split).  The odd last match leaves 64 entries in
    every wave with a hypothesis, the DUP boundary evaluations of one hypothesis come on top: H = 64 -> at least 89 entries,
    one wave's, taken by threads of two waves (the second has no hypothesis); H = 256 -> at least 281 entries of four waves,
    two strides.  No wave's queue (256 entries) can have overflowed while the total stays below 64 x 3 + 256, so every
    parked entry reached the final drain."""
    mode = REPROJECTION_ERROR
    ctx = _ctx(**{"debug.msplit": 1})
    rng = np.random.default_rng(900 + H)
    done = 0
    for _ in range(40):
        if done >= 3:
            break
        prev, cur = _scene(rng, 150)
        n = prev.shape[0]
        i = int(rng.integers(0, n))
        order = np.concatenate([np.arange(n), np.full(DUP - 1, i)])
        rng.shuffle(order)
        m = _identity_matches(order)
        cfg, _ = make_config(EST_FIXED, H, seed=int(rng.integers(1, 1 << 30)))
        h = int(rng.integers(0, H))
        T, valid, _ = oracle.hypothesis_model(cfg, prev, cur, m, h)
        if T is None:
            continue
        err = oracle.eval_errors(T, TUM_FR1_K, prev[i], cur[i])
        e = max(err[1], err[2])
        if not np.isfinite(e) or e <= 1e-9 or e > 1e5:
            continue
        t0, t1 = _boundary(oracle, mode, T, TUM_FR1_K, prev[i], cur[i], e)
        for thr in (t0, t1):
            prm = default_ransac_params(mode)
            prm.minimalNumberOfMatches = 3
            prm.inlierThresholdReprojection = thr
            prm.inlierThresholdEuclidean = 1e5
            got = ctx.debug_ransac_counts(prm, cfg, TUM_FR1_K, prev, cur, m)
            parked, evals = ctx.score_stats()
            want, M = oracle.hypothesis_counts(prm, cfg, TUM_FR1_K, prev, cur, m)
            print("H %d h %d thr %r: parked %d, evaluations %d" % (H, h, thr, parked, evals))
            assert M == n + DUP - 1 and M % 2 == 1
            assert np.array_equal(got, want), (H, h, i, thr)
            assert evals >= H * M, "the decision-exact path did not run"
            # (64 lanes of every wave at the odd last match + the boundary copies; a copy that IS the last match is parked once)
            forced = H + DUP - (1 if order[-1] == i else 0)
            assert forced > H and parked >= forced, ("forced entries were not handed to the value-exact code", parked, forced)
            assert parked < 64 * 3 + 256, ("a queue may have overflowed before the end of the sweep: not the case meant", parked)
        done += 1
    assert done >= 3
    ctx.close()


# ---- all outputs: staged = complete = oracle, one and two pairs -----------------------------------------------------------
_SEQ = {}


def _sequence(frames):
    """The first synthetic sequence of this many frames in which a pair has an odd number of depth-valid matches."""
    if frames not in _SEQ:
        from putslam_amd.device_batch import FrameSetDevice, PairBatchDevice, run_pairs
        prm = _noise_level_params(REPROJECTION_ERROR)
        cfg, _ = make_config(EST_FIXED, 64, seed=1)
        for index in range(16):
            seq = synth.make_sequence(frames, 300, config=3, index=6100 + index, inlier_frac=0.7, noise=NOISE)
            c = api.Context(0)
            fs = FrameSetDevice(seq["desc"], seq["pts"], seq["nkpts"])
            pb = PairBatchDevice(seq["pairs"], fs.max_kpts)
            run_pairs(c, prm, cfg, TUM_FR1_K, fs, pb)
            Mv = [int(s["numMatchesValid"]) for s in pb.download()["stats"]]
            c.close()
            if all(64 <= v <= 300 for v in Mv) and any(v % 2 == 1 for v in Mv):
                _SEQ[frames] = (seq, Mv)
                break
    assert frames in _SEQ
    return _SEQ[frames]


def _run(seq, prm, cfg, prune):
    from putslam_amd.device_batch import FrameSetDevice, PairBatchDevice, run_pairs
    c = _ctx(prune=prune, reorder=1)
    fs = FrameSetDevice(seq["desc"], seq["pts"], seq["nkpts"])
    pb = PairBatchDevice(seq["pairs"], fs.max_kpts)
    run_pairs(c, prm, cfg, TUM_FR1_K, fs, pb)
    g = pb.download()
    parked, evals = c.score_stats()
    c.close()
    return g, parked, evals


@pytest.mark.parametrize("H", [64, 256, 300, 1024])
@pytest.mark.parametrize("frames", [2, 3])
@pytest.mark.parametrize("est", [EST_FIXED, EST_RANSAC])
@pytest.mark.parametrize("mode", [REPROJECTION_ERROR, EUCLIDEAN_AND_REPROJECTION_ERROR])
def test_outputs_staged_and_complete_equal_oracle(oracle, mode, est, frames, H):
    seq, Mv = _sequence(frames)
    P = len(seq["pairs"])
    prm = _noise_level_params(mode)
    cfg, _ = make_config(est, H, seed=4040)
    odd = sum(1 for v in Mv if v % 2 == 1)
    want = []
    for p in range(P):
        cfgp, _ = make_config(est, H, seed=4040 + p)   # pair p of a batch uses seed + p
        want.append(oracle.vo_pairs(prm, cfgp, TUM_FR1_K, seq["desc"], seq["pts"], seq["nkpts"], seq["pairs"][p:p + 1], threads=1))
    for prune in (0, 2):
        g, parked, evals = _run(seq, prm, cfg, prune)
        print("mode %d est %d pairs %d H %d prune %d: M %s, parked %d, evaluations %d" % (mode, est, P, H, prune, Mv, parked, evals))
        assert evals > 0, "the decision-exact path did not run"
        # (the first 64 hypotheses of a pair are swept completely whatever the schedule and the staging: one wave at least
        # meets the odd last match)
        assert parked >= 64 * odd
        for p in range(P):
            cp = want[p]
            n = int(cp["numMatches"][0])
            assert int(g["numMatches"][p]) == n
            assert np.array_equal(g["inlierMask"][p, :n], cp["inlierMask"][0, :n]), (prune, p)
            assert g["pose"][p].tobytes() == cp["pose"][0].tobytes(), (prune, p)
            for f in STAT_FIELDS:
                x, y = g["stats"][p][f], cp["stats"][0][f]
                assert x == y or (np.isnan(x) and np.isnan(y)), (prune, p, f, x, y)
