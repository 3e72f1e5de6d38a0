"""ps_ransac_match_lists on the GPU: RANSAC / USAC over caller-supplied device-resident match lists, byte for byte against per-pair
Context.ransac_rigid3d with seed + p AND against the oracle (tests/track_vo_ref.ransac_lists, which states the rules for the lists
the host form refuses).  Masks are sentinel-filled and checked beyond every count; floats are compared as words."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import track_vo_ref as R  # noqa: E402
from putslam_amd import synth  # noqa: E402
from putslam_amd._abi import (ADAPTIVE_ERROR, DMATCH_DTYPE, EST_FIXED, EST_RANSAC, EST_USAC, EUCLIDEAN_AND_REPROJECTION_ERROR,  # noqa: E402
                              EUCLIDEAN_ERROR, REPROJECTION_ERROR, STATS_DTYPE, TUM_FR1_K, default_ransac_params, make_config)

pytestmark = pytest.mark.gpu

KBLOCK = 256          # the tile of ps_prep_match_lists (kBlock, ps_block.h)
SENT = 0xA5
SEED = 11
MODES = [EUCLIDEAN_ERROR, REPROJECTION_ERROR, EUCLIDEAN_AND_REPROJECTION_ERROR, ADAPTIVE_ERROR]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def scene():
    """Three synthetic pairs of 800, 300 and 64 points with their cross-check matches (the oracle's), and two more previous sets:
    the second pair's with every depth 0, and one whose count will be refused."""
    from oracle import oracle_py
    oracle_py.build()
    prev, cur, lists = [], [], []
    for n, idx in ((800, 4100), (300, 4101), (64, 4102)):
        a, b = synth.make_pair(n, config=2, index=idx)
        prev.append(a["pts"].copy())
        cur.append(b["pts"].copy())
        lists.append(oracle_py.match_hamming256(a["desc"], b["desc"]))
    blind = prev[1].copy()
    blind[:, 2] = 0
    prev += [blind, prev[2].copy()]
    assert len(lists[0]) >= 2 * KBLOCK + 1
    return prev, cur, lists


def bad_indices(m, nprev, ncur):
    """m with matches of index -1, count and beyond spliced in"""
    bad = np.zeros(6, DMATCH_DTYPE)
    bad["queryIdx"] = [-1, 3, nprev, 5, 2 ** 31 - 1, -2 ** 31]
    bad["trainIdx"] = [2, -1, 4, ncur, 1, 0]
    return np.concatenate([bad[:1], m[:20], bad[1:3], m[20:100], bad[3:5], m[100:], bad[5:]])


def directed_batch():
    """(pairs, lists, numMatches) of the directed cases: the compaction's tile seams and the Euclidean record's pair-interleaved tail
    (an odd count), every match depth-invalid, indices outside their sets, counts and set indices the call refuses, a ragged pair"""
    prev, cur, lists = scene()
    rows = [(0, 0, lists[0][:c], None) for c in (0, 1, 2, 3, KBLOCK - 1, KBLOCK, KBLOCK + 1, 2 * KBLOCK + 1, 377)]
    rows += [(3, 1, lists[1], None),                                               # every match depth-invalid
             (1, 1, bad_indices(lists[1], len(prev[1]), len(cur[1])), None),        # indices of -1 and count
             (1, 1, lists[1], -1), (1, 1, lists[1], "cap+1"),                       # numMatches of -1 and cap + 1
             (len(prev), 1, lists[1], None), (1, -1, lists[1], None),               # a pair index outside its group
             (4, 2, lists[2], None),                                                # a set count outside 0 .. capacity
             (2, 2, lists[2], None), (1, 1, lists[1], None)]
    return rows


def run_case(ctx, oracle, rows, prm, estimator, H, pitched, permuted, identity_pairs=False):
    """One call of ps_ransac_match_lists on `rows` against both references."""
    import torch
    from putslam_amd import device_batch as db
    prev, cur, _ = scene()
    if identity_pairs:       # pairs = NULL: set p of both, so the sets are laid out pair by pair
        prev, cur = [prev[a] for a, _, _, _ in rows], [cur[b] for _, b, _, _ in rows]
        rows = [(p, p, m, n) for p, (_, _, m, n) in enumerate(rows)]
    P = len(rows)
    cap = max(len(m) for _, _, m, _ in rows) + 3
    cap_prev, cap_cur = max(len(s) for s in prev) + 2, max(len(s) for s in cur) + 1
    order = np.random.RandomState(3).permutation(P) if permuted else np.arange(P)
    rows = [rows[i] for i in order]
    num = np.array([len(m) if n is None else (cap + 1 if n == "cap+1" else n) for _, _, m, n in rows], np.int32)
    block = np.zeros((P, cap), DMATCH_DTYPE)
    block["queryIdx"] = 2 ** 30            # what lies beyond a list is never followed
    for p, (_, _, m, _) in enumerate(rows):
        block[p, :len(m)] = m
    pairs = np.array([(a, b) for a, b, _, _ in rows], np.int32)
    sets_p = db.PointSets.from_host(prev, "cuda:0", cap_prev, cap_prev * 3 + 5 if pitched else None)
    sets_c = db.PointSets.from_host(cur, "cuda:0", cap_cur, cap_cur * 3 + 7 if pitched else None)
    prev_counts = None
    if not identity_pairs:
        prev_counts = [len(s) for s in prev]
        prev_counts[4] = cap_prev + 1
        sets_p.counts.copy_(torch.from_numpy(np.array(prev_counts, np.int32)))
    out = db.PairResultsDevice(P, cap, "cuda:0")
    out.mask.fill_(SENT)
    out.pose.fill_(float("nan"))
    out.stats.fill_(SENT)
    torch.cuda.synchronize()
    d_matches, d_num = dev(block.view(np.int32).reshape(P, cap, 4)), dev(num)
    db.ransac_match_lists(ctx, prm, make_config(estimator, H, seed=SEED)[0], TUM_FR1_K, sets_p, sets_c, d_matches, d_num,
                          None if identity_pairs else dev(pairs), out)
    got = out.download()
    got["staged_pairs"] = ctx.get_option("last_staged_pairs")      # (before the host form's calls below, one pair each)
    want = R.ransac_lists(oracle, prm, TUM_FR1_K, prev, cur, None if identity_pairs else pairs, [m for _, _, m, _ in rows], num, cap,
                          estimator, H, SEED, prev_counts=prev_counts, prev_cap=cap_prev, cur_cap=cap_cur)
    for p, w in enumerate(want):
        check_pair(ctx, prm, estimator, H, p, got, w, rows[p], prev, cur, prev_counts, cap)
    return got, want


def stats_words(s):
    return np.frombuffer(np.asarray(s, STATS_DTYPE).tobytes(), np.uint8)


def same_stats(a, b, what):
    for f in STATS_DTYPE.names:
        x, y = a[f], b[f]
        assert x == y or (np.isnan(x) and np.isnan(y)), (what, f, a, b)


def check_pair(ctx, prm, estimator, H, p, got, w, row, prev, cur, prev_counts, cap):
    a, b, m, _ = row
    mask = got["inlierMask"][p]
    if w["mask"] is None:
        assert (mask == SENT).all(), p                      # the empty list: no mask byte is written
    else:
        n = len(w["mask"])
        assert mask[:n].tobytes() == w["mask"].tobytes(), p
        assert (mask[n:] == SENT).all(), p
    assert got["pose"][p].tobytes() == np.ascontiguousarray(w["pose"].T).tobytes(), (p, got["pose"][p], w["pose"])
    same_stats(got["stats"][p], w["stats"], p)
    # ... and the host form on the same pair with seed + p (the lists it refuses go through the filter first)
    cfg, _ = make_config(estimator, H, seed=SEED + p)
    if w["mask"] is None:
        h = ctx.ransac_rigid3d(prm, cfg, TUM_FR1_K, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, DMATCH_DTYPE))
        assert h["stats"]["numMatchesIn"] == 0
    else:
        pa, cb = prev[a], cur[b]
        ok = (m["queryIdx"] >= 0) & (m["queryIdx"] < len(pa)) & (m["trainIdx"] >= 0) & (m["trainIdx"] < len(cb))
        h = ctx.ransac_rigid3d(prm, cfg, TUM_FR1_K, pa, cb, m[ok])
        assert mask[:len(m)][ok].tobytes() == h["mask"].tobytes(), p
        h["stats"]["numMatchesIn"] = len(m)
    assert got["pose"][p].tobytes() == np.ascontiguousarray(h["pose"].T).tobytes(), p
    same_stats(got["stats"][p], h["stats"], ("host form", p))


@pytest.fixture
def options(ctx):
    """set_option for the test, the defaults back afterwards"""
    saved = {}

    def set_(name, value):
        saved.setdefault(name, ctx.get_option(name))
        ctx.set_option(name, value)
    yield set_
    for name, value in saved.items():
        ctx.set_option(name, value)


@pytest.mark.parametrize("score", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_directed_lists_ransac(ctx, oracle, options, mode, score):
    """The directed batch under RANSAC <= 487 for every error version and both scoring families; pitched sets and permuted pairs
    for one family, dense sets for the other."""
    options("score", score)
    got, want = run_case(ctx, oracle, directed_batch(), default_ransac_params(mode), EST_RANSAC, 487, pitched=bool(score), permuted=bool(score))
    assert sum(1 for w in want if w["stats"]["accepted"]) >= 5 and sum(1 for w in want if w["mask"] is None) == 5
    if mode == EUCLIDEAN_ERROR and score:
        odd = [w for w in want if w["stats"]["numMatchesValid"] % 2 == 1 and w["stats"]["accepted"]]
        assert odd                                          # the pair-interleaved record's tail is exercised


@pytest.mark.parametrize("mode", [EUCLIDEAN_ERROR, REPROJECTION_ERROR])
def test_directed_lists_usac(ctx, oracle, mode):
    run_case(ctx, oracle, directed_batch(), default_ransac_params(mode), EST_USAC, 600, pitched=False, permuted=True)


@pytest.mark.parametrize("mode", [EUCLIDEAN_ERROR, REPROJECTION_ERROR])
def test_fixed_schedule_staged_scoring_on_three_pairs(ctx, oracle, options, mode):
    """H = 1024 with option prune = 2: the staged scoring, whose per-pair counters the record builder clears."""
    options("prune", 2)
    _, _, lists = scene()
    rows = [(0, 0, lists[0], None), (1, 1, lists[1][:201], None), (2, 2, lists[2], None)]
    got, want = run_case(ctx, oracle, rows, default_ransac_params(mode), EST_FIXED, 1024, pitched=True, permuted=False)
    assert got["staged_pairs"] == 3
    assert all(w["stats"]["accepted"] for w in want[:2])


@pytest.mark.parametrize("P", [1, 5, 70])
def test_pairs_null_and_batch_sizes(ctx, oracle, P):
    """pairs = NULL (set p of both) for 1, 5 (ragged) and 70 pairs: more than the 16 of the wide work-groups elsewhere."""
    _, _, lists = scene()
    rows = [(p % 3, p % 3, lists[p % 3][:len(lists[p % 3]) - 7 * (p // 3)], None) for p in range(P)]
    run_case(ctx, oracle, rows, default_ransac_params(EUCLIDEAN_ERROR), EST_RANSAC, 487, pitched=False, permuted=False, identity_pairs=True)


def golden_call(ctx, name, prm, cfg):
    """(ps_ransac_match_lists on the golden pair's own match list, ps_vo_pairs_device on the same frames)"""
    from putslam_amd import device_batch as db
    G = np.load(os.path.join(HERE, "golden", name + ".npz"))
    n, m = len(G["pts_a"]), G["matches"]
    frames = db.FrameSetDevice(np.stack([G["desc_a"], G["desc_b"]]), np.stack([G["pts_a"], G["pts_b"]]), [n, n])
    batch = db.PairBatchDevice(np.array([[0, 1]], np.int32), n)
    db.run_pairs(ctx, prm, cfg, TUM_FR1_K, frames, batch)
    vo = batch.download()
    block = np.zeros((1, n), DMATCH_DTYPE)
    block[0, :len(m)] = m
    sets_p, sets_c = db.PointSets.from_host([G["pts_a"]], "cuda:0"), db.PointSets.from_host([G["pts_b"]], "cuda:0")
    out = db.ransac_match_lists(ctx, prm, cfg, TUM_FR1_K, sets_p, sets_c, dev(block.view(np.int32).reshape(1, n, 4)),
                                dev(np.array([len(m)], np.int32)))
    return out.download(), vo, m


@pytest.mark.parametrize("mode", MODES)
def test_golden_lists_give_the_bytes_of_vo_pairs(ctx, mode):
    """The golden pairs' match lists fed back in: the bytes ps_vo_pairs_device gives on the same frames -- and a second, smaller call
    on the same context after the larger one (stale records and counters)."""
    prm = default_ransac_params(mode)
    cfg, _ = make_config(EST_RANSAC, 487, seed=1)
    for name in ("pair_n64", "pair_n500", "pair_n64"):
        got, vo, m = golden_call(ctx, name, prm, cfg)
        k = len(m)
        assert vo["numMatches"][0] == k and vo["matches"][0, :k].tobytes() == m.tobytes()
        assert got["inlierMask"][0, :k].tobytes() == vo["inlierMask"][0, :k].tobytes()
        assert got["pose"].tobytes() == vo["pose"].tobytes()
        same_stats(got["stats"][0], vo["stats"][0], name)
        assert vo["stats"][0]["accepted"] == 1


def test_host_form_wrapper_and_refusals(ctx, oracle):
    """Context.ransac_match_lists (numpy in, numpy out) equals the oracle; P == 0 is PS_OK; a sample stream, a NULL and a bad
    stride are refused with outputs untouched."""
    import ctypes as C
    from putslam_amd import api, device_batch as db
    from putslam_amd._abi import PsPointSets
    prev, cur, lists = scene()
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    cfg, _ = make_config(EST_RANSAC, 487, seed=SEED)
    res = ctx.ransac_match_lists(prm, cfg, TUM_FR1_K, prev[:3], cur, [lists[2], lists[0]], pairs=[[2, 2], [0, 0]])
    want = R.ransac_lists(oracle, prm, TUM_FR1_K, prev[:3], cur, [[2, 2], [0, 0]], [lists[2], lists[0]], [len(lists[2]), len(lists[0])],
                          len(lists[0]), EST_RANSAC, 487, SEED)
    for p, w in enumerate(want):
        assert res["inlierMask"][p, :len(w["mask"])].tobytes() == w["mask"].tobytes()
        assert res["pose"][p].tobytes() == np.ascontiguousarray(w["pose"].T).tobytes()
        same_stats(res["stats"][p], w["stats"], p)
    none = ctx.ransac_match_lists(prm, cfg, TUM_FR1_K, prev[:3], cur, [])                 # P == 0: no pair, no row
    assert none["inlierMask"].shape[0] == 0 and none["pose"].shape == (0, 16) and none["stats"].shape == (0,)
    sets_p, sets_c = db.PointSets.from_host(prev[:1], "cuda:0"), db.PointSets.from_host(cur[:1], "cuda:0")
    out = db.PairResultsDevice(1, 8, "cuda:0")
    out.mask.fill_(SENT)
    m, n = dev(np.zeros((1, 8, 4), np.int32)), dev(np.array([3], np.int32))
    ctx.ransac_match_lists_device(prm, cfg, TUM_FR1_K, sets_p.view(), sets_c.view(), None, 0, 0, 0, 8, out.view())      # P == 0
    keep = np.zeros((487, 3), np.uint32)
    bad_cfg, _keep = make_config(EST_RANSAC, 487, seed=1, sample_idx=keep)
    odd = sets_p.view()
    odd.setStride = sets_p.capacity * 12 + 2
    for args in ((prm, bad_cfg, TUM_FR1_K, sets_p.view(), sets_c.view(), None, m.data_ptr(), n.data_ptr(), 1, 8, out.view()),
                 (prm, cfg, TUM_FR1_K, sets_p.view(), sets_c.view(), None, 0, n.data_ptr(), 1, 8, out.view()),
                 (prm, cfg, TUM_FR1_K, odd, sets_c.view(), None, m.data_ptr(), n.data_ptr(), 1, 8, out.view()),
                 (prm, cfg, TUM_FR1_K, sets_p.view(), sets_c.view(), None, m.data_ptr(), n.data_ptr(), 1, 0, out.view())):
        with pytest.raises(api.PsError) as e:
            ctx.ransac_match_lists_device(*args)
        assert e.value.code == -1
    ctx.synchronize()
    assert (out.mask.cpu().numpy() == SENT).all() and not out.pose.cpu().numpy().any()
    assert C.sizeof(PsPointSets) == 32
