"""The restatement of the tracking VO step (tests/track_vo_ref.py) on its scene, without a GPU: the conditions the GPU tests rely on
-- so that they cannot pass vacuously -- and the struct mirrors of the new calls against the built library."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import track_vo_ref as R  # noqa: E402
from putslam_amd._abi import DMATCH_DTYPE, make_config  # noqa: E402

IDENTITY = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def batch():
    return R.batch(1)


def test_accepted_pair_moves_and_both_filters_bite(batch):
    pair, rows, s = batch[0]
    prm = R.params()
    assert pair == (0, 1) and s["stats"]["accepted"] == 1 and not np.array_equal(s["pose"], IDENTITY)
    assert s["stats"]["numInliers"] >= prm.minimalNumberOfMatches and int(s["mask"].sum()) == s["stats"]["numInliers"]
    assert s["stats"]["numMatchesValid"] < s["stats"]["numMatchesIn"] == len(s["kept_idx"])      # the depth gate drops a match
    assert len(s["kept_idx"]) < len(rows["xy"])                                                  # the selection drops a point
    z = s["rows"]["pts"][:, 2]
    assert (z == 0).any() and (z > 6).any()                  # the block without depth and the block beyond 6 m are both hit
    assert (s["status"] == 0).any() and (s["status"] != 0).any()


def test_unrelated_pair_is_rejected_by_the_ratio(batch):
    pair, _, s = batch[3]
    prm = R.params()
    assert pair == (0, R.UNRELATED)
    assert s["stats"]["numMatchesValid"] >= prm.minimalNumberOfMatches                           # not by minimalNumberOfMatches
    assert s["stats"]["bestInlierRatio"] < prm.minimalInlierRatioThreshold and s["stats"]["accepted"] == 0
    assert np.array_equal(s["pose"], IDENTITY) and not s["mask"].any()


def test_two_previous_points_give_identity(batch):
    _, rows, s = batch[4]
    assert len(rows["xy"]) == 2 and np.array_equal(s["pose"], IDENTITY) and s["stats"]["accepted"] == 0
    assert s["stats"]["bestHypothesis"] == -1


def test_every_pair_tracks_something_and_the_capacities_differ(batch):
    sizes = [len(rows["xy"]) for _, rows, _ in batch]
    assert min(sizes) == 2 and max(sizes) > 256                 # more than one block of 256 rows
    for _, _, s in batch:
        assert len(s["kept_idx"]) > 0
        assert np.array_equal(s["rows"]["xy"], s["next_pts"][s["kept_idx"]])


def test_the_batch_for_a_capacity_of_64_has_every_kind_of_pair():
    B = R.batch(1, 64)
    assert len(B) == 5 and max(len(rows["xy"]) for _, rows, _ in B) == 64
    assert [int(s["stats"]["accepted"]) for _, _, s in B] == [1, 1, 1, 0, 0]
    assert all(not np.array_equal(s["pose"], IDENTITY) for _, _, s in B[:3])
    assert B[3][0] == (0, R.UNRELATED) and len(B[3][2]["kept_idx"]) > 0 and len(B[4][1]["xy"]) == 2
    for _, rows, s in B[:3]:
        assert s["stats"]["numMatchesValid"] < s["stats"]["numMatchesIn"] < len(rows["xy"])     # both filters bite


def test_chaining_through_the_rows_equals_rows_built_by_hand(oracle, batch):
    """(0, 1) -> (1, 2): the rows the first step leaves, taken as they are, against the same rows put together from the pieces."""
    _, rows0, s01 = batch[0]
    chained = R.step(oracle, 1, (1, 2), s01["rows"], 0)
    kept = s01["kept_idx"]
    xy = s01["next_pts"][kept]
    und = oracle.remove_image_distortion(xy, R.K, R.DIST5)
    hand = dict(xy=xy, pts=oracle.keypoints2Dto3D(und, R.depths()[1], R.K, R.DEPTH_SCALE))
    for n in R.CARRIED:
        hand[n] = rows0[n][kept]
    by_hand = R.step(oracle, 1, (1, 2), hand, 0)
    for k in ("next_pts", "status", "err", "kept_idx", "mask", "pose"):
        assert chained[k].tobytes() == by_hand[k].tobytes(), k
    assert chained["matches"].tobytes() == by_hand["matches"].tobytes()
    for k in ("xy", "xy_undist", "pts") + R.CARRIED:
        assert chained["rows"][k].tobytes() == by_hand["rows"][k].tobytes(), k
    assert chained["stats"]["accepted"] == 1 and chained["stats"]["numMatchesIn"] == len(chained["kept_idx"])
    # the carried columns are the first frame's, two selections deep
    assert np.array_equal(chained["rows"]["det_dist"], rows0["det_dist"][kept][chained["kept_idx"]])


def test_refill_step():
    assert R.refill_step([200, 160, 149, 170]) == 2 and R.refill_step([150, 150]) == 2 and R.refill_step([]) == 0


def test_the_filter_in_front_of_the_oracle(oracle, batch):
    """An index outside its set is dropped like a depth-invalid match: the results are those of the list without it, the mask keeps
    the list's positions and numMatchesIn its length; a refused count or set gives the empty list and no mask."""
    _, rows, s = batch[0]
    prm = R.params()
    cfg, _ = make_config(0, R.HYP, seed=R.SEED)
    m = s["matches"].copy()
    bad = np.zeros(3, DMATCH_DTYPE)
    bad["queryIdx"], bad["trainIdx"] = [-1, 5, len(rows["pts"])], [3, len(s["rows"]["pts"]), 0]
    mixed = np.concatenate([m[:10], bad[:1], m[10:50], bad[1:], m[50:]])
    r = R.ransac_list(oracle, prm, cfg, R.K, rows["pts"], s["rows"]["pts"], mixed)
    keep = np.ones(len(mixed), bool)
    keep[[10, 51, 52]] = False
    assert r["mask"][keep].tobytes() == s["mask"].tobytes() and not r["mask"][~keep].any()
    assert r["pose"].tobytes() == s["pose"].tobytes() and r["stats"]["numMatchesIn"] == len(mixed)
    assert r["stats"]["numMatchesValid"] == s["stats"]["numMatchesValid"] and r["stats"]["pointInlierRatio"] == s["stats"]["pointInlierRatio"]
    e = R.ransac_list(oracle, prm, cfg, R.K, rows["pts"], s["rows"]["pts"], m, valid=False)
    assert e["mask"] is None and np.array_equal(e["pose"], IDENTITY) and e["stats"]["numMatchesIn"] == 0 and e["stats"]["accepted"] == 0


def test_struct_mirrors_match_the_library():
    from putslam_amd import _lib
    L = _lib.load()
    sizes = _lib.struct_sizes_track_vo()
    assert len(sizes) == 6
    for name, size in sizes.items():
        assert getattr(L, "ps_abi_sizeof_" + name)() == size, name
