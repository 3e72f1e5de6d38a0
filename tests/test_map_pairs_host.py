"""Batched map matching, the parts that need no GPU: ps_map_sphere_bound, the PsMapBatch layout, and the CPU reference
helper (tests/map_pairs_ref.py) on hand-made cases -- the capacity rule and the retry ladder's selection."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_pairs_ref as mref  # noqa: E402

from putslam_amd._abi import DMATCH_DTYPE, EST_RANSAC, EUCLIDEAN_ERROR, TUM_FR1_K, default_ransac_params  # noqa: E402


def _bound(r):
    from putslam_amd import api
    return np.float32(api.map_sphere_bound(r))


def _radii():
    rng = np.random.default_rng(20261016)
    ladder = [mref.ladder_try(0.12, 0.55, k)[0] for k in range(1, 11)]
    rnd = list(np.exp(rng.uniform(np.log(1e-6), np.log(1e6), 200)))
    return ladder + rnd


def test_sphere_bound_is_the_least_float_whose_root_reaches_the_radius():
    """(float)sqrt(s) < r  <=>  s < B: the rounded root of the float just below B is below r, that of B is not
    (numpy's float32 square root is correctly rounded, like sqrtf)."""
    for r in _radii():
        B = _bound(r)
        assert B > 0 and np.isfinite(B), r
        below = np.nextafter(B, np.float32(-np.inf))
        assert float(np.sqrt(below, dtype=np.float32)) < r, (r, B)
        assert not float(np.sqrt(B, dtype=np.float32)) < r, (r, B)


def test_sphere_bound_special_values():
    assert _bound(0.0) == 0 and _bound(-1.0) == 0 and _bound(float("nan")) == 0 and _bound(-0.0) == 0
    assert _bound(1.9e19) == np.inf and _bound(float("inf")) == np.inf
    assert np.isfinite(_bound(1.8e19))
    assert _bound(1e-30) > 0


@pytest.mark.parametrize("radius", [0.12, 0.16, 0.3, 1.0])
def test_oracle_decides_at_the_bound_like_the_bound_says(oracle, radius):
    """Two points whose squared distance (the kernel's float sum) is exactly B are no candidates, one ulp below they are."""
    B = _bound(radius)
    desc = np.zeros((1, 32), np.uint8)
    lvl = np.zeros(1, np.int32)
    found = 0
    for want, inside in ((B, False), (np.nextafter(B, np.float32(-np.inf)), True)):
        q = mref.sphere_edge_points(B, want)
        assert q is not None, (radius, want)      # (the search is deterministic: both points exist for these radii)
        found += 1
        m = oracle.match_xyz(np.zeros((1, 3), np.float32), desc, lvl, q.reshape(1, 3), desc, lvl, radius, 0.55)
        assert (len(m) == 1) == inside, (radius, want, q)
    assert found == 2, radius


def test_map_batch_layout_matches_library():
    from putslam_amd import _lib
    from putslam_amd._abi import PsMapBatch
    L = _lib.load()
    assert L.ps_abi_sizeof_map_batch() == C.sizeof(PsMapBatch) == _lib.struct_sizes()["map_batch"]
    assert "ps_map_pairs_device" in _lib.EXPORTED and "ps_match_xyz_device" in _lib.EXPORTED
    # entry points refuse a missing context without a GPU
    assert L.ps_map_pairs_device(None, None, None, None, None, None) == -1
    assert L.ps_match_xyz_device(None, None, None, None) == -1


def test_python_ladder_rules_are_the_reference_helper_s():
    from putslam_amd import api
    for k in range(1, 12):
        assert api.ladder_try(0.12, 0.55, k) == mref.ladder_try(0.12, 0.55, k)
    assert mref.ladder_try(0.12, 0.55, 1) == (0.12, 0.55)
    assert mref.ladder_try(0.12, 0.55, 3) == (0.12 + 0.02 * 2, 0.55 - 0.05 * 2)
    # (the tenth try's ratio is the double 0.55 - 0.05 * 9 = 0.10000000000000003, as the reference computes it; the floor holds from 11 on)
    assert mref.ladder_try(0.12, 0.55, 10)[1] == 0.55 - 0.05 * 9 and mref.ladder_try(0.12, 0.55, 11)[1] == 0.1
    nan = float("nan")
    for seq in ([0.05, 0.2, 0.3], [0.0, 0.01, 0.09], [nan, nan, 0.1], [nan, nan], [0.1], [0.0999999, nan, 0.5, 0.05]):
        assert api.ladder_pick(seq) == mref.ladder_pick(seq)


def test_ladder_pick():
    nan = float("nan")
    assert mref.ladder_pick([0.05, 0.2, 0.3]) == 1            # the first try that reaches 0.1
    assert mref.ladder_pick([0.1, 0.0]) == 0                  # "not below": 0.1 itself ends the loop
    assert mref.ladder_pick([0.0, 0.01, 0.09]) == 2           # none does: the last
    assert mref.ladder_pick([nan, nan, 0.4, 0.9]) == 2        # no matches = -1.0 < 0.1
    assert mref.ladder_pick([nan, nan]) == 1
    assert mref.ladder_pick([0.5], 0.1) == 0
    assert mref.ladder_pick([0.2, 0.6], 0.5) == 1


def _tiny_scene():
    # a view of 4 features on 4 keypoints of a frame (exact positions, equal descriptors), and an empty view
    cur = np.array([[0, 0, 2], [0.5, 0, 2], [0, 0.5, 2], [0.5, 0.5, 2.5]], np.float32)
    frames = dict(pos=cur[None], desc=np.full((1, 4, 32), 7, np.uint8), level=np.zeros((1, 4), np.int32),
                  nkpts=np.array([4], np.int32), cap=4)
    vpos = np.zeros((3, 4, 3), np.float32)
    vpos[0] = cur
    vpos[2] = cur + np.float32(10.0)      # far from everything
    views = dict(pos=vpos, desc=np.full((3, 4, 32), 7, np.uint8), level=np.zeros((3, 4), np.int32),
                 nkpts=np.array([4, 0, 4], np.int32), cap=4)
    return views, frames


def test_reference_helper_capacity_and_no_candidate_rules(oracle):
    views, frames = _tiny_scene()
    ref = mref.Ref(oracle, views, frames)
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    prm.minimalNumberOfMatches = 3
    full = ref.pair(prm, EST_RANSAC, 64, 5, TUM_FR1_K, 0, 0, 0.12, 0.55, 8)
    assert full["numMatches"] == 4 and [tuple(m)[:3] for m in full["matches"]] == [(j, j, -1) for j in range(4)]
    assert int(full["stats"]["numMatchesIn"]) == 4
    # overflow: -(count), identity, nothing accepted, the estimator saw no matches
    over = ref.pair(prm, EST_RANSAC, 64, 5, TUM_FR1_K, 0, 0, 0.12, 0.55, 3)
    assert over["numMatches"] == -4 and len(over["matches"]) == 0 and len(over["mask"]) == 0
    assert over["pose"].tolist() == np.eye(4, dtype=np.float32).reshape(16).tolist()
    assert int(over["stats"]["accepted"]) == 0 and int(over["stats"]["numInliers"]) == 0
    assert int(over["stats"]["numMatchesIn"]) == 0 and np.isnan(over["stats"]["pointInlierRatio"])
    # no candidate (an empty view, a view far away): 0 matches, identity, NaN -> the ladder's -1.0
    for v in (1, 2):
        none = ref.pair(prm, EST_RANSAC, 64, 5, TUM_FR1_K, v, 0, 0.12, 0.55, 8)
        assert none["numMatches"] == 0 and none["matches"].dtype == DMATCH_DTYPE and len(none["matches"]) == 0
        assert none["pose"].tolist() == np.eye(4, dtype=np.float32).reshape(16).tolist()
        assert np.isnan(none["stats"]["pointInlierRatio"]) and int(none["stats"]["accepted"]) == 0
        assert mref.ladder_pick([float(none["stats"]["pointInlierRatio"])] * 3) == 2
    # a batch: pair p is seeded seed + p
    b = ref.batch(prm, EST_RANSAC, 64, 5, TUM_FR1_K, [(0, 0), (1, 0), (0, 0)], [0.12, 0.12, 0.14], 0.55, 8)
    assert [x["numMatches"] for x in b] == [4, 0, 4]
    assert mref.canon_stats(b[0]["stats"]) == mref.canon_stats(full["stats"])
