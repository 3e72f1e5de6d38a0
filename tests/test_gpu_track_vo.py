"""The tracking VO step on the GPU (putslam_amd/csrc/ps_track_vo.h): ps_assemble_tracked and ps_track_vo_pairs against the
restatement of Matcher::trackKLT (tests/track_vo_ref.py), batched against pair by pair, and device_batch.run_tracked_sequences
against the chain frame by frame.  Everything is compared byte for byte -- floats as words; where the expected float is a NaN the
device's is a NaN too -- and sentinel-filled outputs are checked beyond every count."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import track_vo_ref as R  # noqa: E402
from track_vo_util import (PAD, dev, depth_block, device_scene, fill_sentinel, rows_to_device, same_bits, same_stats,  # noqa: E402
                           untouched)
from putslam_amd._abi import DMATCH_DTYPE, EST_RANSAC, frame_geometry, klt_params, make_config, track_vo_params  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, COLS = R.ROWS, R.COLS
CAP = 300                                        # two blocks of 256 rows
COUNTS = [65, CAP, 64, 0, 1, -1, CAP + 1]
FRAMES = [3, 1, 5, 0, -1, 1, 0]                  # the depth frame of every pair: permuted, and two outside the set of five
ROW_NAMES = ("xy", "xy_undist", "pts") + R.CARRIED


def geometry():
    return frame_geometry(R.K, R.DIST5, R.DEPTH_SCALE)


def edge_positions(oracle):
    """Two distorted positions that UNDISTORT to u == cols in an inner row (the next row's first pixel, never the padding) and to
    v == rows (no pixel: depth 0), found on a grid: this wide camera's distortion has no closed inverse near the border."""
    y, x = np.mgrid[-10:ROWS + 10:0.25, -10:COLS + 10:0.25]
    grid = np.stack([x.ravel(), y.ravel()], 1).astype(np.float32)
    und = oracle.remove_image_distortion(grid, R.K, R.DIST5)
    u, v = np.rint(und[:, 0]), np.rint(und[:, 1])
    right = np.nonzero((u == COLS) & (v > 30) & (v < 60) & (np.abs(und[:, 0] - COLS) < 0.3))[0][0]
    below = np.nonzero((v == ROWS) & (u > 10) & (u < 30) & (np.abs(und[:, 1] - ROWS) < 0.3))[0][0]
    return grid[[right, below]]


def tracked_inputs(oracle, seed=13):
    """next_pts (P, CAP, 2): positions over and around the image with named ones in the first rows of every pair -- the first two
    UNDISTORT to u == cols in an inner row (the next row's first pixel, never the padding) and to v == rows (depth 0) --, kept
    (P, CAP) permutations that keep the named rows, and the previous rows' columns."""
    rng = np.random.RandomState(seed)
    P = len(COUNTS)
    pts = (rng.rand(P, CAP, 2) * [COLS + 20, ROWS + 20] - 10).astype(np.float32)
    named = np.concatenate([edge_positions(oracle),
                            np.float32([[np.nan, 10.0], [10.0, np.inf], [-3.0, -0.3], [COLS - 1.0, ROWS - 1.0], [0.0, 0.0], [1e30, 5.0]])])
    pts[:, :len(named)] = named
    kept = np.stack([rng.permutation(CAP) for _ in range(P)]).astype(np.int32)
    for p in range(P):        # the named positions are output rows 0 .. of every pair that has that many
        rest = [i for i in kept[p] if i >= len(named)]
        kept[p] = np.concatenate([np.arange(len(named)), rest])
    cols = dict(angle=(rng.rand(P, CAP) * 360).astype(np.float32), response=rng.randn(P, CAP).astype(np.float32),
                octave=rng.randint(0, 8, size=(P, CAP)).astype(np.int32), det_dist=rng.rand(P, CAP) * 5)
    return pts, kept, cols, len(named)


def sentinel_rows(P, cap, carried=R.CARRIED, xy_undist=True):
    from putslam_amd import device_batch as db
    out = db.TrackedRows(P, cap, "cuda:0", carried)
    if not xy_undist:
        out.xy_undist = None
    for n in ROW_NAMES:
        if getattr(out, n) is not None:
            fill_sentinel(getattr(out, n))
    fill_sentinel(out.counts)
    return out


def test_assemble_tracked_equals_the_restatement(ctx, oracle):
    """Counts at the block seams, -1 and capacity + 1 (count -1, nothing written); a depth set whose rows and frames are padded
    with 0xEEEE; depth frames permuted and outside the set (depth 0); indices outside 0 .. capacity-1 (zero rows); rows beyond a
    count keep the sentinel; the carried columns are the previous rows' by index."""
    import torch
    from putslam_amd import device_batch as db
    pts, kept, cols, named = tracked_inputs(oracle)
    P = len(COUNTS)
    safe = kept.copy()
    kept[1, 290], kept[1, 291], kept[0, 20] = CAP, -1, 2 ** 31 - 1
    deps = R.depths()
    view = depth_block(deps)
    prev = db.TrackedRows(P, CAP, "cuda:0")
    for n in R.CARRIED:
        getattr(prev, n).copy_(dev(cols[n]))
    out = sentinel_rows(P, CAP)
    torch.cuda.synchronize()
    db.assemble_tracked(ctx, geometry(), view, dev(np.array(FRAMES, np.int32)), dev(pts), dev(kept), dev(np.array(COUNTS, np.int32)), prev, out)
    torch.cuda.synchronize()
    got = out.download()
    assert got["counts"].tolist() == [n if 0 <= n <= CAP else -1 for n in COUNTS]
    seen_pad = np.float32(PAD / R.DEPTH_SCALE)
    for p, n in enumerate(COUNTS):
        n = n if 0 <= n <= CAP else 0
        g = FRAMES[p]
        want = R.tracked_rows(oracle, pts[p], safe[p, :n], deps[g] if 0 <= g < len(deps) else None, {k: v[p] for k, v in cols.items()})
        for name in ROW_NAMES:
            w = want[name].copy()
            if p == 1 and n:
                w[290:292] = 0
            if p == 0 and n:
                w[20] = 0
            same_bits(got[name][p, :n], w.astype(got[name].dtype), (name, p))
            assert untouched(got[name][p, n:]), (name, p)
        assert not (got["pts"][p, :n, 2] == seen_pad).any(), p
        if not 0 <= g < len(deps) and n:
            assert (got["pts"][p, :n, 2] == 0).all(), p                 # no depth frame: depth 0
    # the named positions did what their names say (pair 1 holds them all, in depth frame 1)
    w = R.tracked_rows(oracle, pts[1], safe[1, :named], deps[1])
    und = w["xy_undist"][:2]
    row = oracle.round_size(und[0][1], ROWS)
    assert oracle.round_size(und[0][0], COLS) == COLS and 0 <= row < ROWS - 1 and oracle.round_size(und[1][1], ROWS) == ROWS
    assert w["pts"][0, 2] == np.float32(deps[1][row + 1, 0] / R.DEPTH_SCALE) and deps[1][row + 1, 0] != 0      # the next row's first pixel
    assert w["pts"][1, 2] == 0 and np.isnan(w["pts"][2, 0]) and w["pts"][2, 2] == 0
    assert (got["pts"][1, :CAP, 2] > 6).any() and (got["pts"][1, :CAP, 2] == 0).any()


@pytest.mark.parametrize("carried", [(), ("det_dist",), ("angle", "octave"), R.CARRIED])
def test_assemble_tracked_optional_columns(ctx, oracle, carried):
    """Each carried column is wanted exactly where the previous rows have it; xy_undist may be absent; the others are what they
    were.  A carried column without its output is refused."""
    import torch
    from putslam_amd import api, device_batch as db
    from putslam_amd._abi import PsTrackedCarry
    pts, kept, cols, _ = tracked_inputs(oracle, 5)
    pts, kept, counts = pts[:2, :64].copy(), np.stack([np.random.RandomState(f).permutation(64) for f in range(2)]).astype(np.int32), [64, 37]
    deps = R.depths()
    prev = None
    if carried:
        prev = db.TrackedRows(2, 64, "cuda:0", carried)
        for n in carried:
            getattr(prev, n).copy_(dev(cols[n][:2, :64]))
    out = sentinel_rows(2, 64, carried, xy_undist=bool(carried))
    torch.cuda.synchronize()
    frames = dev(np.array([2, 4], np.int32))
    db.assemble_tracked(ctx, geometry(), depth_block(deps), frames, dev(pts), dev(kept), dev(np.array(counts, np.int32)), prev, out)
    torch.cuda.synchronize()
    got = out.download()
    assert sorted(got) == sorted(["counts", "xy", "pts"] + (["xy_undist"] if carried else []) + list(carried))
    for p, n in enumerate(counts):
        want = R.tracked_rows(oracle, pts[p], kept[p, :n], deps[[2, 4][p]], {k: cols[k][p, :64] for k in carried})
        for name in got:
            if name != "counts":
                same_bits(got[name][p, :n], want[name].astype(got[name].dtype), (name, p))
                assert untouched(got[name][p, n:]), (name, p)
    if not carried:
        stray = PsTrackedCarry(None, None, None, out.pts.data_ptr())       # detDist carried, no output for it
        with pytest.raises(api.PsError) as e:
            ctx.assemble_tracked_device(geometry(), db.DepthSet(depth_block(deps), ROWS, COLS), frames.data_ptr(), dev(pts).data_ptr(),
                                        dev(kept).data_ptr(), dev(np.array(counts, np.int32)).data_ptr(), 2, 64, stray, out.rows_struct())
        assert e.value.code == -1


# ------------------------------------------------------------------------------------------------------------ the whole step
def sentinel_out(P, cap, carried=R.CARRIED):
    from putslam_amd import device_batch as db
    out = db.TrackVoDevice(P, cap, "cuda:0", carried)
    for t in (out.next_pts, out.status, out.err, out.kept_idx, out.num_matches, out.mask, out.pose, out.stats):
        fill_sentinel(t)
    out.matches.fill_(0xA5)
    out.rows = sentinel_rows(P, cap, carried)
    return out


def expected_ransac(oracle, rows, s, p, seed=R.SEED):
    """the estimator of pair p at position p of a batch (seed + p) on the restatement's rows and matches"""
    cfg, _ = make_config(EST_RANSAC, R.HYP, seed=seed + p)
    return R.ransac_list(oracle, R.params(), cfg, R.K, rows["pts"], s["rows"]["pts"], s["matches"])


def check_step(oracle, got, p, rows, s, seed_pos=None):
    """every output of PsTrackVoOut for pair p of `got` equals the restatement's step `s` from `rows`"""
    n, k = len(rows["xy"]), len(s["kept_idx"])
    same_bits(got["next_pts"][p, :n], s["next_pts"], ("next_pts", p))
    assert got["status"][p, :n].tobytes() == s["status"].tobytes(), p
    same_bits(got["err"][p, :n], s["err"], ("err", p))
    for name in ("next_pts", "status", "err"):
        assert untouched(got[name][p, n:]), (name, p)
    assert got["numMatches"][p] == k and got["rows"]["counts"][p] == k, (p, got["numMatches"][p], k)
    assert got["matches"][p, :k].tobytes() == s["matches"].tobytes(), p
    assert (got["matches"][p, k:].view(np.uint8) == 0xA5).all(), p
    assert got["kept_idx"][p, :k].tolist() == s["kept_idx"].tolist() and untouched(got["kept_idx"][p, k:]), p
    for name in ROW_NAMES:
        same_bits(got["rows"][name][p, :k], s["rows"][name].astype(got["rows"][name].dtype), (name, p))
        assert untouched(got["rows"][name][p, k:]), (name, p)
    r = s if seed_pos is None else expected_ransac(oracle, rows, s, seed_pos)
    assert got["inlierMask"][p, :k].tobytes() == r["mask"].tobytes() and untouched(got["inlierMask"][p, k:]), p
    assert got["pose"][p].tobytes() == np.ascontiguousarray(r["pose"].T).tobytes(), (p, got["pose"][p], r["pose"])
    same_stats(got["stats"][p], r["stats"], p)


def run_batch(ctx, cn, cap, scene=None):
    """ps_track_vo_pairs on the five pairs of the restatement's batch for capacity `cap`"""
    import torch
    from putslam_amd import device_batch as db
    pyr, depth = scene or device_scene(ctx, cn)
    B = R.batch(cn, cap)
    pairs = np.array([b[0] for b in B], np.int32)
    rows = rows_to_device([b[1] for b in B], cap)
    out = sentinel_out(len(B), cap)
    torch.cuda.synchronize()
    cfg, _ = make_config(EST_RANSAC, R.HYP, seed=R.SEED)
    db.track_vo_pairs(ctx, pyr, depth, geometry(), dev(pairs), rows, R.params(), cfg, track_vo_params(R.ERR_THRESHOLD, R.MIN_DIST), out=out)
    torch.cuda.synchronize()
    return out.download()


@pytest.mark.parametrize("cap", [64, 300])
@pytest.mark.parametrize("cn", [1, 3])
def test_track_vo_pairs_equals_the_chain(ctx, oracle, cn, cap):
    """Five pairs as one ragged batch, at capacity 300 (260, 64, 150, 200 and 2 previous points: more than one block of rows) and at
    capacity 64 (64, 48, 63, 64 and 2: less than one) -- accepted pairs, a pair on an unrelated texture that is rejected, a pair
    below minimalNumberOfMatches: every output of PsTrackVoOut, for grey and three-channel images."""
    B = R.batch(cn, cap)
    assert len(B) == 5 and max(len(rows["xy"]) for _, rows, _ in B) <= cap
    got = run_batch(ctx, cn, cap)
    for p, (_, rows, s) in enumerate(B):
        check_step(oracle, got, p, rows, s)
    assert [int(x) for x in got["stats"]["accepted"]] == [1, 1, 1, 0, 0]


def test_batched_equals_pair_by_pair_equals_the_host_form(ctx, oracle):
    """Pair p of the batch = a call of its own with seed + p = ps_track_vo_pair on host arrays: every output, byte for byte."""
    import torch
    from putslam_amd import device_batch as db
    B = R.batch(1)
    pyr, depth = device_scene(ctx, 1)
    batched = run_batch(ctx, 1, 300, (pyr, depth))
    for p, (pair, rows, s) in enumerate(B):
        cap = max(len(rows["xy"]), 1)
        out = sentinel_out(1, cap)
        torch.cuda.synchronize()
        cfg, _ = make_config(EST_RANSAC, R.HYP, seed=R.SEED + p)
        db.track_vo_pairs(ctx, pyr, depth, geometry(), dev(np.array([pair], np.int32)), rows_to_device([rows], cap), R.params(), cfg,
                          track_vo_params(R.ERR_THRESHOLD, R.MIN_DIST), out=out)
        torch.cuda.synchronize()
        one = out.download()
        n, k = len(rows["xy"]), int(one["numMatches"][0])
        assert k == batched["numMatches"][p]
        for name, m in (("next_pts", n), ("status", n), ("err", n), ("matches", k), ("kept_idx", k), ("inlierMask", k)):
            assert one[name][0, :m].tobytes() == batched[name][p, :m].tobytes(), (name, p)
        for name in ROW_NAMES:
            assert one["rows"][name][0, :k].tobytes() == batched["rows"][name][p, :k].tobytes(), (name, p)
        assert one["pose"][0].tobytes() == batched["pose"][p].tobytes() and one["stats"][0].tobytes() == batched["stats"][p].tobytes()
        # ... and the host form on numpy arrays: uploads included, synchronous
        imgs = R.images(1)
        h = ctx.track_vo_pair(imgs[pair[0]], imgs[pair[1]], R.depths()[pair[1]], geometry(), rows, R.params(), cfg,
                              track_vo_params(R.ERR_THRESHOLD, R.MIN_DIST), klt_params(R.WIN, R.LEVELS, R.MAX_COUNT, R.EPS))
        assert len(h["kept_idx"]) == k
        for name, m, key in (("next_pts", n, "next_pts"), ("status", n, "status"), ("err", n, "err"), ("matches", k, "matches"),
                             ("kept_idx", k, "kept_idx"), ("inlierMask", k, "mask")):
            assert h[key].tobytes() == one[name][0, :m].tobytes(), (name, p)
        for name in ROW_NAMES:
            assert h["rows"][name].tobytes() == one["rows"][name][0, :k].tobytes(), (name, p)
        assert np.ascontiguousarray(h["pose"].T).tobytes() == one["pose"][0].tobytes() and h["stats"].tobytes() == one["stats"][0].tobytes()


def test_depth_frame_given_and_counts_of_zero_and_minus_one(ctx, oracle):
    """depthFrame names another frame than the pair's current slot; prevCounts 0 gives the identity and no matches
    (matcher.cpp:147-148); a count the selection refuses gives rows of count -1 and the results of the empty list."""
    import torch
    from putslam_amd import device_batch as db
    pyr, depth = device_scene(ctx, 1)
    pair, rows, _ = R.batch(1)[1]
    s = R.step(oracle, 1, pair, rows, 0, depth_frame=0)
    cap = 64
    prev = rows_to_device([rows, rows, rows], cap)
    prev.counts.copy_(dev(np.array([len(rows["xy"]), 0, cap + 1], np.int32)))
    out = sentinel_out(3, cap)
    torch.cuda.synchronize()
    cfg, _ = make_config(EST_RANSAC, R.HYP, seed=R.SEED)
    db.track_vo_pairs(ctx, pyr, depth, geometry(), dev(np.array([pair] * 3, np.int32)), prev, R.params(), cfg,
                      track_vo_params(R.ERR_THRESHOLD, R.MIN_DIST), depth_frame=dev(np.array([0, 0, 0], np.int32)), out=out)
    torch.cuda.synchronize()
    got = out.download()
    check_step(oracle, got, 0, rows, s)
    assert not np.array_equal(s["rows"]["pts"], R.batch(1)[1][2]["rows"]["pts"])          # the other depth frame shows
    ident = np.eye(4, dtype=np.float32)
    assert got["numMatches"].tolist() == [len(s["kept_idx"]), 0, -1] and got["rows"]["counts"].tolist() == [len(s["kept_idx"]), 0, -1]
    for p in (1, 2):
        assert got["pose"][p].tobytes() == ident.tobytes() and got["stats"][p]["accepted"] == 0 and got["stats"][p]["numMatchesIn"] == 0
        assert untouched(got["inlierMask"][p]) and untouched(got["rows"]["pts"][p]) and untouched(got["kept_idx"][p])


def test_remove_too_close_features_is_refused(ctx):
    """removeTooCloseFeatures = 1: PS_ERR_UNSUPPORTED with a text, outputs untouched."""
    import torch
    from putslam_amd import api, device_batch as db
    pyr, depth = device_scene(ctx, 1)
    pair, rows, _ = R.batch(1)[1]
    out = sentinel_out(1, 64)
    torch.cuda.synchronize()
    cfg, _ = make_config(EST_RANSAC, R.HYP, seed=R.SEED)
    with pytest.raises(api.PsError) as e:
        db.track_vo_pairs(ctx, pyr, depth, geometry(), dev(np.array([pair], np.int32)), rows_to_device([rows], 64), R.params(), cfg,
                          track_vo_params(R.ERR_THRESHOLD, R.MIN_DIST, 1), out=out)
    assert e.value.code == -5 and "removeTooCloseFeatures" in str(e.value)
    ctx.synchronize()
    torch.cuda.synchronize()
    for t in (out.next_pts, out.status, out.err, out.kept_idx, out.num_matches, out.mask, out.pose, out.stats, out.rows.pts, out.rows.counts):
        assert untouched(t)


def test_run_tracked_sequences_equals_the_chain(ctx, oracle):
    """Two sequences of three frames in lockstep -- (0, 1, 2) from 260 points and (1, 2, 3) from 150 --, the rows handed on where
    they lie: every step equals the chain frame by frame, and the refill steps are the restatement's."""
    from putslam_amd import device_batch as db
    pyr, depth = device_scene(ctx, 1)
    B = R.batch(1)
    first = [B[0][1], R.first_rows(oracle, 150, 5, 1)]
    frames = np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    cfg, _ = make_config(EST_RANSAC, R.HYP, seed=R.SEED)
    steps, refill = db.run_tracked_sequences(ctx, pyr, depth, rows_to_device(first, 300), frames, geometry(), R.params(), cfg,
                                             track_vo_params(R.ERR_THRESHOLD, R.MIN_DIST), minimal_tracked_features=R.MINIMAL_TRACKED)
    rows, counts = list(first), [[], []]
    for k in range(2):
        got = steps[k].download()
        for s_ in range(2):
            want = B[0][2] if (k, s_) == (0, 0) else R.step(oracle, 1, (int(frames[s_, k]), int(frames[s_, k + 1])), rows[s_], s_)
            n, kk = len(rows[s_]["xy"]), len(want["kept_idx"])
            same_bits(got["next_pts"][s_, :n], want["next_pts"], (k, s_))
            assert got["numMatches"][s_] == kk and got["matches"][s_, :kk].tobytes() == want["matches"].tobytes()
            for name in ROW_NAMES:
                same_bits(got["rows"][name][s_, :kk], want["rows"][name].astype(got["rows"][name].dtype), (name, k, s_))
            assert got["inlierMask"][s_, :kk].tobytes() == want["mask"].tobytes()
            assert got["pose"][s_].tobytes() == np.ascontiguousarray(want["pose"].T).tobytes()
            same_stats(got["stats"][s_], want["stats"], (k, s_))
            rows[s_] = want["rows"]
            counts[s_].append(kk)
    assert refill.tolist() == [R.refill_step(c) for c in counts]
    assert sorted(set(refill.tolist())) != [2]                  # a refill is due somewhere: the return value is exercised
    assert DMATCH_DTYPE.itemsize == 16
