"""Closing the tracking VO step on the GPU (ps_track_close.h): ps_track_close_pairs and ps_track_candidates against the restatement
of Matcher::trackKLT's second half (tests/track_close_ref.py), byte for byte -- floats as words; where the expected float is a NaN
the device's is one too.  Every output block is filled with 0xEE before a call and must still hold it beyond every count, and
everywhere for a pair the call refuses (counts -1).  The scene is the 150 x 200 images of tests/frame_assembly_ref.py; the thresholds
are small (minimalTrackedFeatures 20, distance 5) so that every case fits 24 tracked rows and 260 candidates; the seam cases of the
merge (test_merge_seams_*) bring blocks of their own: 520 tracked rows and 1100 candidates."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import frame_assembly_ref as A  # noqa: E402
import orb_ref as O  # noqa: E402
import track_close_ref as C  # noqa: E402
from image_frontend_util import upload_images  # noqa: E402
from track_vo_util import dev, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
MINIMAL, DIST = 20, 5.0
CAP, CCAP, OCAP = 24, 260, 288          # tracked rows, candidates, output rows (two blocks of 256) a pair
ROW_NAMES = tuple(n for n, _, _ in C.COLUMNS)


@pytest.fixture(scope="module")
def ctx():
    from putslam_amd import api
    return api.Context(0)


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle_py
    oracle_py.build()
    return oracle_py


# ---------------------------------------------------------------------------------------------------------------- the cases
def tracked_sets():
    """name -> (rows, the count the device is told)"""
    # (no two of them within 0.0001 px of each other: tests/test_track_close_ref_host.py shows what the reference's walk does there)
    border = [(np.nextafter(f32(31), f32(0)), 60), (31, 70), (np.nextafter(f32(A.COLS - 31), f32(0)), 80), (A.COLS - 31, 90),
              (70, np.nextafter(f32(31), f32(0))), (80, 31), (90, np.nextafter(f32(A.ROWS - 31), f32(0))), (100, A.ROWS - 31), (30.99, 100)]
    t19 = C.random_rows(19, 1)
    t19["xy"][:9] = np.array(border, f32)
    t19["xy"][9:13] = [[60, 50], [80, 50], [100, 50], [120, 50]]      # describable, whatever the level says
    t19["octave"][9:13] = [100, -1, 8, 3]                             # outside the level table; two inside it that no detector emits
    t19["pts"][12] = 0                                                # depth 0: the quotient is not finite
    t19["pts"][13, 2] = 0                                             # ... and a point beside the axis with depth 0
    out = {"t0": (C.empty_rows(), 0), "t19": (t19, 19), "t20": (C.random_rows(20, 2), 20), "t21": (C.random_rows(21, 3), 21),
           "bad-1": (C.random_rows(5, 4), -1), "bad+1": (C.random_rows(5, 4), CAP + 1)}
    return out


def candidate_frames():
    """[(rows, the count the device is told)]: counts 0, 1, 64, 65, 256, 257 (half of each a pixel from a row of t19), all rejected,
    all accepted, the special frame, and two whose count is refused"""
    t19 = tracked_sets()["t19"][0]
    out = [(C.near_and_far_candidates(t19, n, 20 + n), n) for n in (0, 1, 64, 65, 256, 257)]
    rej = C.random_rows(40, 30)
    rej["xy_undist"] = (t19["xy_undist"][np.arange(40) % 19] + f32(1.0)).astype(f32)
    out.append((rej, 40))                                                                        # 6: every candidate near a row of t19
    gy, gx = np.mgrid[0:12, 0:20]
    grid = np.stack([gx.ravel() * 8 + 20, gy.ravel() * 8 + 20], axis=1).astype(f32)
    out.append((C.rows_at(grid, 31), len(grid)))                                                 # 7: 240 candidates 8 px apart: all accepted
    special = [(50, 60), (53, 60), (57, 60),                         # the greedy triple for d = 5: A, B near A, C near B only
               (100, 100), (103, 104),                               # exactly 5 apart: accepted
               (140, 100), (np.nextafter(f32(143), f32(0)), 104),    # one ulp closer: rejected
               (np.nan, np.nan), (30.99, 70)]                        # a NaN (appended, not described), a border row
    out.append((C.rows_at(special, 32), len(special)))                                           # 8
    out.append((C.random_rows(5, 33), -1))                                                       # 9, 10: refused counts
    out.append((C.random_rows(5, 34), CCAP + 1))
    return out


SPECIAL_ACCEPTED = [0, 2, 3, 4, 5, 7, 8]

# (tracked set, candidate frame): every case of the list above; -1 and 99 name no frame
PAIRS = [("t0", 7), ("t0", 8), ("t0", -1), ("t19", 0), ("t19", 1), ("t19", 2), ("t19", 3), ("t19", 4), ("t19", 5), ("t19", 6),
         ("t19", -1), ("t19", 99), ("t20", 4), ("t21", 5), ("t20", -1), ("bad-1", 2), ("bad+1", 2), ("t19", 9), ("t19", 10), ("t20", 9),
         ("t0", 0), ("t0", 5)]
FIVE = [1, 5, 9, 12, 21]                # the batch of five: no refused pair (its rows go into ps_vo_pairs_device)

_WANT = {}


def pyramids(cn):
    if ("pyr", cn) not in _WANT:
        _WANT["pyr", cn] = [O.pyramid(img, C.SCALE_FACTOR, C.N_LEVELS) for img in A.images(cn)[:2]]
    return _WANT["pyr", cn]


def want(spec, slot, cn):
    """the restatement's result for one pair (None: refused), computed once"""
    key = (spec, slot, cn)
    if key not in _WANT:
        tset, cframes = tracked_sets(), candidate_frames()
        rows, n = tset[spec[0]]
        res = None
        if 0 <= n <= CAP:
            cand = None
            due = n < MINIMAL
            if due and 0 <= spec[1] < len(cframes):
                crow, cn_ = cframes[spec[1]]
                cand = C.take(crow, np.arange(max(min(cn_, len(crow["xy"])), 0))) if 0 <= cn_ <= CCAP else "refused"
            if not isinstance(cand, str):
                res = C.close(rows, cand, pyramids(cn)[slot], CAP, MINIMAL, DIST)
        _WANT[key] = res
    return _WANT[key]


# ---------------------------------------------------------------------------------------------------------------- device side
def fill_ee(*tensors):
    import torch
    for t in tensors:
        t.view(torch.uint8).fill_(0xEE)


def is_ee(a):
    a = a if isinstance(a, np.ndarray) else a.cpu().numpy()
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xEE).all())


def put_rows(block, p, rows, n):
    """rows [0, n) of pair / frame p of a TrackedRows / FrameRowsDevice"""
    for name in ROW_NAMES:
        if n > 0:
            getattr(block, name)[p, :n] = dev(np.asarray(rows[name])[:n])


def device_tracked(specs):
    from putslam_amd import device_batch as db
    t = db.TrackedRows(len(specs), CAP, "cuda:0")
    fill_ee(*[getattr(t, n) for n in ROW_NAMES])
    tset = tracked_sets()
    for p, (name, _) in enumerate(specs):
        rows, n = tset[name]
        put_rows(t, p, rows, min(len(rows["xy"]), CAP))
    t.counts.copy_(dev(np.array([tset[name][1] for name, _ in specs], np.int32)))
    return t


def device_candidates():
    from putslam_amd import device_batch as db
    frames = candidate_frames()
    c = db.FrameRowsDevice(len(frames), CCAP, "cuda:0")
    fill_ee(*[getattr(c, n) for n in ROW_NAMES])
    for f, (rows, n) in enumerate(frames):
        put_rows(c, f, rows, min(len(rows["xy"]), CCAP))
    c.nkpts.copy_(dev(np.array([n for _, n in frames], np.int32)))
    return c


def closed_out(P, cap=OCAP):
    from putslam_amd import device_batch as db
    out = db.ClosedRows(P, cap, "cuda:0")
    fill_ee(out.desc, out.src_idx, out.refill, out.rows.counts, *[getattr(out.rows, n) for n in ROW_NAMES])
    return out


def device_pyramids(ctx, cn):
    from putslam_amd import device_batch as db
    pyr = db.OrbPyramids(ctx, A.ROWS, A.COLS, cn, 2)
    pyr.build(upload_images(A.images(cn)[:2], True))
    return pyr


def check(got, specs, slots, cn, what):
    for p, (spec, slot) in enumerate(zip(specs, slots)):
        w = want(spec, slot, cn)
        if w is None:
            assert got["rows"]["counts"][p] == -1, (what, p, spec)
            assert is_ee(got["refill"][p:p + 1]) and is_ee(got["desc"][p]) and is_ee(got["src_idx"][p]), (what, p, spec)
            assert all(is_ee(got["rows"][n][p]) for n in ROW_NAMES), (what, p, spec)
            continue
        k = len(w["xy"])
        assert got["rows"]["counts"][p] == k and got["refill"][p] == w["refill"], (what, p, spec, got["rows"]["counts"][p], k)
        same_bits(got["desc"][p, :k], w["desc"], (what, p, "desc"))
        same_bits(got["src_idx"][p, :k], w["src_idx"], (what, p, "src_idx"))
        assert is_ee(got["desc"][p, k:]) and is_ee(got["src_idx"][p, k:]), (what, p, spec)
        for n, dt, _ in C.COLUMNS:
            same_bits(got["rows"][n][p, :k], np.asarray(w[n], dt), (what, p, n))
            assert is_ee(got["rows"][n][p, k:]), (what, p, n)


def run(ctx, tc, pyr, specs, slots, cand, tp=None, out=None, cap=OCAP):
    import torch
    from putslam_amd import device_batch as db
    from putslam_amd._abi import track_close_params
    out = out or closed_out(len(specs), cap)
    torch.cuda.synchronize()
    res = db.track_close_pairs(ctx, tc, pyr, dev(np.array(slots, np.int32)), device_tracked(specs), cand,
                               None if cand is None else dev(np.array([c for _, c in specs], np.int32)),
                               tp or track_close_params(MINIMAL, DIST), out=out)
    torch.cuda.synchronize()
    return res


STAT_FIELDS = ("numMatchesIn", "numMatchesValid", "bestHypothesis", "bestInlierCount", "iterationsRun", "numInliers", "accepted",
               "bestInlierRatio", "pointInlierRatio")


def same_pairs(got, want_):
    """The device's pair results equal the oracle's: matches, masks, every field of the statistics, the poses."""
    assert got["numMatches"].tolist() == want_["numMatches"].tolist()
    for q, m in enumerate(want_["numMatches"].tolist()):
        assert got["matches"][q, :m].tobytes() == want_["matches"][q, :m].tobytes(), q
        assert got["inlierMask"][q, :m].tobytes() == want_["inlierMask"][q, :m].tobytes(), q
        for f in STAT_FIELDS:
            a, b = got["stats"][q][f], want_["stats"][q][f]
            assert a == b or (np.isnan(a) and np.isnan(b)), (q, f, a, b)
    assert got["pose"].tobytes() == want_["pose"].tobytes()


def fe_params(p, levels):
    from putslam_amd._abi import front_end_params, orb_detect_params, orb_params
    det = orb_detect_params(p["n_features"], p["scale_factor"], p["n_levels"], p["fast_threshold"], p["grid_rows"], p["grid_cols"], p["max_features"])
    return front_end_params(det, orb_params(p["scale_factor"], levels), A.DBSCAN_EPS)


# ---------------------------------------------------------------------------------------------------------------- the tests
def test_the_cases_are_what_they_are_named(oracle):
    """(CPU work, but the restatement needs the library's host level function beside the images)"""
    assert C.close(tracked_sets()["t0"][0], candidate_frames()[8][0], pyramids(1)[0], CAP, MINIMAL, DIST)["merged_src"].tolist() == \
        [CAP + i for i in SPECIAL_ACCEPTED]
    assert len(want(("t0", 7), 0, 1)["merged_src"]) == 240 and want(("t19", 6), 0, 1)["merged_src"].tolist() == list(range(19))
    assert want(("t20", 4), 0, 1)["refill"] == 0 and want(("t19", 99), 0, 1)["refill"] == 2 and want(("t19", 9), 0, 1) is None
    t19 = want(("t19", -1), 0, 1)
    assert t19["level"][9] == -1 and t19["level"][12] == 0 and sorted(t19["src_idx"].tolist())[:5] == [1, 2, 5, 6, 10]
    assert t19["walk"].tolist() == t19["kept"].tolist()
    for n, f in ((64, 2), (65, 3), (256, 4), (257, 5)):
        acc = len(want(("t19", f), 0, 1)["merged_src"]) - 19
        assert 0 < acc < n - n // 2, (n, acc)              # some of the free half lie on each other: the greedy rule works inside a tile and across tiles


@pytest.mark.parametrize("P", [1, 5, 70])
def test_batch_equals_the_restatement(ctx, P):
    """P = 1 / 5 / 70 ragged: every case of PAIRS (70 pairs run through it three times with the slots alternating)"""
    from putslam_amd import device_batch as db
    idx = {1: [8], 5: FIVE, 70: [i % len(PAIRS) for i in range(70)]}[P]
    specs, slots = [PAIRS[i] for i in idx], [(i // 3) % 2 for i in range(P)]
    tc, pyr = db.TrackClose(ctx, 70, OCAP), device_pyramids(ctx, 1)
    got = run(ctx, tc, pyr, specs, slots, device_candidates()).download()
    check(got, specs, slots, 1, P)
    if P == 70:
        assert sorted(set(got["refill"][got["rows"]["counts"] >= 0].tolist())) == [0, 1, 2]
        assert int((got["rows"]["counts"] == -1).sum()) == sum(want(s, sl, 1) is None for s, sl in zip(specs, slots)) == 12
    tc.close()
    pyr.close()


def test_colour_pair_by_pair_and_no_candidates(ctx):
    """Three channels; the batch of five equals five calls of one pair, block for block; cand = None closes every due pair with
    refill 2; a larger out-capacity than needed changes nothing."""
    import torch
    from putslam_amd import device_batch as db
    specs, slots = [PAIRS[i] for i in FIVE], [0, 1, 1, 0, 1]
    tc, pyr, cand = db.TrackClose(ctx, 5, OCAP + 12), device_pyramids(ctx, 3), device_candidates()
    whole = run(ctx, tc, pyr, specs, slots, cand)
    check(whole.download(), specs, slots, 3, "colour")
    for p in range(5):
        one = run(ctx, tc, pyr, specs[p:p + 1], slots[p:p + 1], cand)
        for a, b in [(one.desc, whole.desc), (one.src_idx, whole.src_idx), (one.refill, whole.refill), (one.rows.counts, whole.rows.counts)] + \
                [(getattr(one.rows, n), getattr(whole.rows, n)) for n in ROW_NAMES]:
            assert torch.equal(a[0:1].view(torch.uint8), b[p:p + 1].view(torch.uint8)), p
    wide = run(ctx, tc, pyr, specs, slots, cand, cap=OCAP + 12).download()
    check(wide, specs, slots, 3, "wide")
    none = run(ctx, tc, pyr, specs, slots, None, cap=CAP).download()
    check(none, [(t, -1) for t, _ in specs], slots, 3, "no candidates")
    assert none["refill"].tolist() == [2, 2, 2, 0, 2]
    tc.close()
    pyr.close()


# ---- the seams of the merge: blocks of their own size (tests/track_close_ref.py: SEAM_*; the premises are asserted on the
# restatement in tests/test_track_close_ref_host.py::test_seam_cases_cross_every_tile_seam_of_the_merge)
SEAM_PAIRS = [(nt, nc) for nt in C.SEAM_TRACKED for nc in C.SEAM_CANDIDATES]
SEAM_OCAP = C.SEAM_CAP + C.SEAM_CCAP


def seam_want(nt, nc, slot):
    key = ("seam", nt, nc, slot)
    if key not in _WANT:
        tracked, cand = C.seam_case(nt, nc)
        _WANT[key] = C.close(tracked, cand, pyramids(1)[slot], C.SEAM_CAP, C.SEAM_MINIMAL, C.SEAM_MIN_DIST)
    return _WANT[key]


def seam_run(ctx, tc, pyr, pairs, slots):
    """ps_track_close_pairs on the seam cases `pairs`, one candidate frame per pair, every block filled with 0xEE first"""
    import torch
    from putslam_amd import device_batch as db
    from putslam_amd._abi import track_close_params
    P = len(pairs)
    t, c, out = db.TrackedRows(P, C.SEAM_CAP, "cuda:0"), db.FrameRowsDevice(P, C.SEAM_CCAP, "cuda:0"), closed_out(P, SEAM_OCAP)
    fill_ee(*[getattr(t, n) for n in ROW_NAMES])
    fill_ee(*[getattr(c, n) for n in ROW_NAMES])
    for p, (nt, nc) in enumerate(pairs):
        tracked, cand = C.seam_case(nt, nc)
        put_rows(t, p, tracked, nt)
        put_rows(c, p, cand, nc)
    t.counts.copy_(dev(np.array([nt for nt, _ in pairs], np.int32)))
    c.nkpts.copy_(dev(np.array([nc for _, nc in pairs], np.int32)))
    torch.cuda.synchronize()
    db.track_close_pairs(ctx, tc, pyr, dev(np.array(slots, np.int32)), t, c, dev(np.arange(P, dtype=np.int32)),
                         track_close_params(C.SEAM_MINIMAL, C.SEAM_MIN_DIST), out=out)
    torch.cuda.synchronize()
    return out


def seam_check(got, pairs, slots, what):
    for p, ((nt, nc), slot) in enumerate(zip(pairs, slots)):
        w = seam_want(nt, nc, slot)
        k = len(w["xy"])
        assert got["rows"]["counts"][p] == k and got["refill"][p] == w["refill"] == 1, (what, nt, nc, got["rows"]["counts"][p], k)
        same_bits(got["src_idx"][p, :k], w["src_idx"], (what, nt, nc, "src_idx"))
        same_bits(got["desc"][p, :k], w["desc"], (what, nt, nc, "desc"))
        assert is_ee(got["desc"][p, k:]) and is_ee(got["src_idx"][p, k:]), (what, nt, nc)
        for n, dt, _ in C.COLUMNS:
            same_bits(got["rows"][n][p, :k], np.asarray(w[n], dt), (what, nt, nc, n))
            assert is_ee(got["rows"][n][p, k:]), (what, nt, nc, n)


@pytest.mark.parametrize("nt,nc", SEAM_PAIRS)
def test_merge_seams_pair_by_pair(ctx, nt, nc):
    """255 / 256 / 257 / 513 tracked rows against 513 / 1100 candidates, candidates 512 .. 600 copies of 0 .. 88 a pixel away: the
    tracked-row loop and the accepted-candidate loop take their second and third trips, and a candidate of the third tile is
    rejected because of one accepted in the first.  srcIdx, the closed rows, desc and refill equal the restatement."""
    from putslam_amd import device_batch as db
    tc, pyr = db.TrackClose(ctx, 1, SEAM_OCAP), device_pyramids(ctx, 1)
    slot = (nt + nc) % 2
    seam_check(seam_run(ctx, tc, pyr, [(nt, nc)], [slot]).download(), [(nt, nc)], [slot], "one pair")
    tc.close()
    pyr.close()


def test_merge_seams_batch_equals_pair_by_pair(ctx):
    """The eight seam cases as one call equal the restatement, and block for block the eight calls of one pair."""
    import torch
    from putslam_amd import device_batch as db
    slots = [(nt + nc) % 2 for nt, nc in SEAM_PAIRS]
    tc, pyr = db.TrackClose(ctx, len(SEAM_PAIRS), SEAM_OCAP), device_pyramids(ctx, 1)
    whole = seam_run(ctx, tc, pyr, SEAM_PAIRS, slots)
    seam_check(whole.download(), SEAM_PAIRS, slots, "batch")
    for p, pair in enumerate(SEAM_PAIRS):
        one = seam_run(ctx, tc, pyr, [pair], slots[p:p + 1])
        for a, b in [(one.desc, whole.desc), (one.src_idx, whole.src_idx), (one.refill, whole.refill), (one.rows.counts, whole.rows.counts)] + \
                [(getattr(one.rows, n), getattr(whole.rows, n)) for n in ROW_NAMES]:
            assert torch.equal(a[0:1].view(torch.uint8), b[p:p + 1].view(torch.uint8)), pair
    tc.close()
    pyr.close()


def test_closed_rows_are_a_frame_set_for_vo_pairs(ctx, oracle):
    """desc, pts and counts of the closed rows go into ps_vo_pairs_device where they lie: the oracle's match + RANSAC on the
    restatement's arrays"""
    from putslam_amd import device_batch as db
    from putslam_amd._abi import EST_RANSAC, default_ransac_params, make_config
    specs, slots = [PAIRS[i] for i in FIVE], [0, 0, 1, 1, 0]
    tc, pyr = db.TrackClose(ctx, 5, OCAP), device_pyramids(ctx, 1)
    closed = run(ctx, tc, pyr, specs, slots, device_candidates())
    frames = [want(s, sl, 1) for s, sl in zip(specs, slots)]
    desc, pts, n = A.frame_set(frames, OCAP)
    assert closed.nkpts.cpu().numpy().tolist() == n.tolist() and (n > 0).all()
    pairs = np.array([[0, 1], [1, 2], [2, 3], [3, 4], [4, 0]], np.int32)
    prm = default_ransac_params(0)
    cfg, _ = make_config(EST_RANSAC, 487, 1)
    batch = db.PairBatchDevice(pairs, OCAP, "cuda:0")
    db.run_pairs(ctx, prm, cfg, A.K, closed, batch)
    same_pairs(batch.download(), oracle.vo_pairs(prm, cfg, A.K, desc, pts, n, pairs))
    tc.close()
    pyr.close()


def test_refusals_leave_the_outputs_untouched(ctx):
    import torch
    from putslam_amd import api, device_batch as db
    from putslam_amd._abi import track_close_params
    specs, slots = [PAIRS[i] for i in FIVE], [0, 1, 0, 1, 0]
    tc, pyr, cand = db.TrackClose(ctx, 5, OCAP), device_pyramids(ctx, 1), device_candidates()
    small = db.TrackClose(ctx, 4, OCAP)
    out = closed_out(5)
    rows = device_tracked(specs)
    frames = dev(np.array([c for _, c in specs], np.int32))
    sl = dev(np.array(slots, np.int32))
    torch.cuda.synchronize()

    def refused(code, text, **kw):
        a = dict(tc=tc, pyr=pyr, slots=sl, rows=rows, cand=cand, cand_frame=frames, tp=track_close_params(MINIMAL, DIST), out=out)
        a.update(kw)
        with pytest.raises(api.PsError) as e:
            db.track_close_pairs(ctx, **a)
        assert e.value.code == code and text in str(e.value), str(e.value)

    refused(-5, "removeTooCloseFeatures", tp=track_close_params(MINIMAL, DIST, 1))
    refused(-1, "maxPairs", tc=small)
    no_octave = device_tracked(specs)
    no_octave.octave = None
    refused(-1, "every column", rows=no_octave)
    no_dist = device_tracked(specs)
    no_dist.det_dist = None
    refused(-1, "every column", rows=no_dist)
    refused(-1, "outCapacity", out=closed_out(5, CAP + CCAP - 1))
    refused(-1, "maxRows", out=closed_out(5, OCAP + 4))
    with pytest.raises(api.PsError) as e:      # a candidate block without candFrame
        ctx.track_close_pairs_device(tc.handle, pyr.handle, sl.data_ptr(), track_close_params(MINIMAL, DIST), rows.rows_struct(),
                                     db.PsTrackCandidates(cand.xy.data_ptr(), cand.xy_undist.data_ptr(), cand.pts.data_ptr(),
                                                          cand.angle.data_ptr(), cand.response.data_ptr(), cand.octave.data_ptr(),
                                                          cand.det_dist.data_ptr(), cand.nkpts.data_ptr(), cand.num_frames, CCAP),
                                     None, 5, CAP, OCAP, out.out_struct())
    assert e.value.code == -1 and "candFrame" in str(e.value)
    ctx.synchronize()
    torch.cuda.synchronize()
    for t in [out.desc, out.src_idx, out.refill, out.rows.counts] + [getattr(out.rows, n) for n in ROW_NAMES]:
        assert is_ee(t)
    # P == 0 is fine and writes nothing
    ctx.track_close_pairs_device(tc.handle, pyr.handle, None, track_close_params(MINIMAL, DIST), rows.rows_struct(), None, None, 0, CAP, OCAP,
                                 out.out_struct())
    torch.cuda.synchronize()
    assert is_ee(out.rows.counts)
    for h in (tc, small, pyr):
        h.close()


@pytest.mark.parametrize("cn", [1, 3], ids=["grey", "colour"])
def test_candidates_equal_the_sandbox_of_the_reference(ctx, oracle, cn):
    """ps_track_candidates on the four frames (a texture, the texture moved, noise, a constant image with no key point) = detect,
    DBScan, undistort, back-project and the detection distances of the restatement, 0xEE beyond every count; nothing is described."""
    import torch
    from putslam_amd import device_batch as db
    from putslam_amd._abi import frame_geometry
    name, p, levels = A.CASES[0]
    imgs, deps = A.images(cn), A.depths()
    fe = db.FrontEnd(ctx, A.ROWS, A.COLS, cn, 4, fe_params(p, levels))
    out = db.FrameRowsDevice(4, A.CAPACITY, "cuda:0")
    fill_ee(out.desc, out.nkpts, out.src_idx, *[getattr(out, n) for n in ROW_NAMES])
    torch.cuda.synchronize()
    db.track_candidates(ctx, fe, upload_images(imgs, True), dev(np.stack(deps).view(np.int16)), frame_geometry(A.K, A.DIST5, A.DEPTH_SCALE),
                        A.CAPACITY, out=out)
    torch.cuda.synchronize()
    got = out.download()
    counts = []
    for f in range(4):
        w = C.candidates(oracle, imgs[f], deps[f], p, A.DBSCAN_EPS)
        k = len(w["xy"])
        counts.append(k)
        assert got["nkpts"][f] == k
        for n, dt, _ in C.COLUMNS:
            same_bits(got[n][f, :k], np.asarray(w[n], dt), (cn, f, n))
            assert is_ee(got[n][f, k:]), (cn, f, n)
    assert counts[0] > 20 and counts[3] == 0 and is_ee(got["desc"])
    fe.close()


# ---------------------------------------------------------------------------------------------------------------- the chain
CHAIN_FRAMES = [[0, 1, 0, 1], [1, 0, 1, 0]]      # two sequences over the texture and the texture moved by (2, 3)
CHAIN_MINIMAL, CHAIN_SEED = 45, 7                # sequence 0 tracks 46, 44, 45 rows: its refill is due at step 1 and only there


def chain_reference(oracle):
    if "chain" not in _WANT:
        name, p, levels = A.CASES[0]
        imgs, deps = A.images(1), A.depths()
        rows0 = [C.candidates(oracle, imgs[f[0]], deps[f[0]], p, A.DBSCAN_EPS) for f in CHAIN_FRAMES]
        _WANT["chain"] = (rows0, C.tracked_vo(oracle, imgs, deps, CHAIN_FRAMES, rows0, A.CAPACITY, A.CAPACITY, p, A.DBSCAN_EPS,
                                              CHAIN_MINIMAL, CHAIN_SEED))
    return _WANT["chain"]


def test_chain_of_tracked_frames_equals_the_restatement_under_both_policies(ctx, oracle):
    """ps_track_vo_pairs -> ps_track_close_pairs -> the next frame, three steps on two sequences: sequence 0 refills at step 1 (44
    tracked rows, two of 46 candidates merged), sequence 1 never.  run_tracked_vo equals the restatement step by step under
    candidates="always" and candidates="due", and the two policies leave the same bytes."""
    import torch
    import track_vo_ref as V
    from putslam_amd import device_batch as db
    from putslam_amd._abi import EST_RANSAC, frame_geometry, make_config, track_close_params, track_vo_params
    from track_vo_util import same_stats
    rows0, ref = chain_reference(oracle)
    assert [[e["closed"]["refill"] for e in seq] for seq in ref] == [[0, 1, 0], [0, 0, 0]]
    assert len(ref[0][1]["step"]["rows"]["xy"]) == 44 and len(ref[0][1]["closed"]["level"]) == 46
    name, p, levels = A.CASES[0]
    imgs, deps = A.images(1), A.depths()
    dimg, ddep = upload_images(imgs, False), dev(np.stack(deps).view(np.int16))
    S, K, cap = 2, 3, A.CAPACITY
    klt = db.KltPyramids(ctx, A.ROWS, A.COLS, 1, 4, V.WIN, V.LEVELS)
    klt.build(dimg)
    orb = db.OrbPyramids(ctx, A.ROWS, A.COLS, 1, 4)
    orb.build(dimg)
    fe = db.FrontEnd(ctx, A.ROWS, A.COLS, 1, S, fe_params(p, levels))
    tc = db.TrackClose(ctx, S, cap * (K + 1))
    first = db.TrackedRows(S, cap, "cuda:0")
    for s, r in enumerate(rows0):
        put_rows(first, s, r, len(r["xy"]))
    first.counts.copy_(dev(np.array([len(r["xy"]) for r in rows0], np.int32)))
    cfg, _ = make_config(EST_RANSAC, V.HYP, seed=CHAIN_SEED)
    geo = frame_geometry(A.K, A.DIST5, A.DEPTH_SCALE)
    runs = {}
    for policy in ("always", "due"):
        steps, closed, counts, refill = db.run_tracked_vo(ctx, klt, orb, fe, tc, dimg, ddep, first, CHAIN_FRAMES, geo, V.params(), cfg,
                                                          track_vo_params(V.ERR_THRESHOLD, C.MIN_DIST),
                                                          close_tp=track_close_params(CHAIN_MINIMAL, C.MIN_DIST), cand_capacity=cap,
                                                          candidates=policy)
        torch.cuda.synchronize()
        assert refill.T.tolist() == [[0, 1, 0], [0, 0, 0]], policy
        for k in range(K):
            got_s, got_c = steps[k].download(), closed[k].download()
            for s in range(S):
                w = ref[s][k]
                n, m = len(w["step"]["rows"]["xy"]), len(w["closed"]["xy"])
                assert got_s["rows"]["counts"][s] == n and got_c["rows"]["counts"][s] == m == counts[k, s], (policy, k, s)
                for name_, dt, _ in C.COLUMNS:
                    same_bits(got_s["rows"][name_][s, :n], np.asarray(w["step"]["rows"][name_], dt), (policy, k, s, name_))
                    same_bits(got_c["rows"][name_][s, :m], np.asarray(w["closed"][name_], dt), (policy, k, s, "closed", name_))
                same_bits(got_c["desc"][s, :m], w["closed"]["desc"], (policy, k, s, "desc"))
                same_bits(got_c["src_idx"][s, :m], w["closed"]["src_idx"], (policy, k, s, "src_idx"))
                same_bits(got_s["pose"][s].reshape(4, 4).T, w["step"]["pose"], (policy, k, s, "pose"))
                assert got_s["inlierMask"][s, :n].tobytes() == w["step"]["mask"].tobytes(), (policy, k, s)
                same_stats(got_s["stats"][s], w["step"]["stats"], (policy, k, s))
        runs[policy] = [t.clone() for k in range(K) for t in
                        [steps[k].pose, steps[k].mask, steps[k].rows.counts, closed[k].desc, closed[k].src_idx, closed[k].refill,
                         closed[k].rows.counts] + [getattr(closed[k].rows, n_) for n_ in ROW_NAMES]]
    assert all(torch.equal(a, b) for a, b in zip(runs["always"], runs["due"]))
    for h in (klt, orb, fe, tc):
        h.close()


def test_host_form_equals_the_chain_reference(ctx, oracle):
    """ps_track_close_pair (uploads, the pyramid build and -- only when due -- the sandbox included) on the tracked rows of three
    steps of the chain = the restatement: a step that is not due, the step that refills, and a refill from nothing (no rows at all:
    matcher.cpp:147-148, then :213-279).  A candidate's srcIdx counts from max(n, 1)."""
    from putslam_amd._abi import frame_geometry, track_close_params
    rows0, ref = chain_reference(oracle)
    name, p, levels = A.CASES[0]
    imgs, deps = A.images(1), A.depths()
    geo, tp = frame_geometry(A.K, A.DIST5, A.DEPTH_SCALE), track_close_params(CHAIN_MINIMAL, C.MIN_DIST)
    cases = [(ref[0][0]["step"]["rows"], CHAIN_FRAMES[0][1], ref[0][0]["closed"], A.CAPACITY),
             (ref[0][1]["step"]["rows"], CHAIN_FRAMES[0][2], ref[0][1]["closed"], 2 * A.CAPACITY)]
    nothing = C.close(C.empty_rows(), C.candidates(oracle, imgs[1], deps[1], p, A.DBSCAN_EPS), pyramids(1)[1], 1, CHAIN_MINIMAL)
    cases.append((C.empty_rows(), 1, nothing, 1))
    assert [c[2]["refill"] for c in cases] == [0, 1, 1] and len(nothing["xy"]) > 20
    for tracked, frame, w, cap in cases:
        n = len(tracked["xy"])
        got = ctx.track_close_pair(imgs[frame], deps[frame], geo, tracked, fe_params(p, C.N_LEVELS), tp)
        assert got["refill"] == w["refill"] and len(got["desc"]) == len(w["xy"])
        same_bits(got["desc"], w["desc"], "desc")
        src = w["src_idx"].astype(np.int64)
        same_bits(got["src_idx"], np.where(src >= cap, src - cap + max(n, 1), src).astype(np.int32), "src_idx")
        for name_, dt, _ in C.COLUMNS:
            same_bits(got["rows"][name_], np.asarray(w[name_], dt), name_)
