"""tests/track_close_ref.py -- the restatement of Matcher::trackKLT's second half (matcher.cpp:213-381) -- shows, on the CPU alone,
every property the GPU tests of ps_track_close_pairs rely on: a refill that merges some candidates and not all, the greedy rule
where it differs from the all-earlier one, the bound at exactly the distance, a NaN candidate, levels with ties, the border, and
that the position-matching walk of :359-375 selects what the description's keptIdx names.  No GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import exclusion_ref_py as X  # noqa: E402
import frame_assembly_ref as A  # noqa: E402
import orb_ref as O  # noqa: E402
import track_close_ref as C  # noqa: E402

f32 = np.float32
CAP = 64


def pyramid():
    if not hasattr(pyramid, "p"):
        pyramid.p = O.pyramid(A.images(1)[1], C.SCALE_FACTOR, C.N_LEVELS)
    return pyramid.p


def accepted(out, cap=CAP):
    """the candidates among the merged rows"""
    return out["merged_src"][out["merged_src"] >= cap] - cap


def test_struct_sizes_match_the_library():
    from putslam_amd import _lib
    L = _lib.load()
    sizes = _lib.struct_sizes_track_close()
    assert sizes == dict(track_candidates=72, track_close_params=16, track_close_out=88)
    for name, size in sizes.items():
        assert getattr(L, "ps_abi_sizeof_" + name)() == size and "ps_abi_sizeof_" + name in _lib.EXPORTED, name
    for name in ("ps_track_candidates", "ps_track_close_create", "ps_track_close_destroy", "ps_track_close_pairs"):
        assert hasattr(L, name) and name in _lib.EXPORTED, name


def test_due_refill_merges_some_candidates_and_not_all():
    tracked = C.random_rows(40, 1)
    cand = C.near_and_far_candidates(tracked, 60, 2)
    out = C.close(tracked, cand, pyramid(), CAP)
    acc = accepted(out)
    assert out["refill"] == 1 and 10 < len(acc) < 30 and not (acc % 2 == 0).any()        # every other one lies on a tracked row
    assert len(acc) < 30                                                                # ... and some of the rest on each other
    assert (np.diff(out["merged_src"][40:]) > 0).all() and (out["merged_src"][:40] == np.arange(40)).all()
    assert 0 < len(out["xy"]) < 40 + len(acc)                                           # the description drops rows too
    assert (out["src_idx"] >= CAP).any() and (out["src_idx"] < 40).any()
    # not due: the candidates are ignored; due without candidates: closed without the refill
    same = C.close(tracked, cand, pyramid(), CAP, minimal=40)
    none = C.close(tracked, None, pyramid(), CAP)
    assert same["refill"] == 0 and none["refill"] == 2 and len(accepted(same)) == 0
    assert same["desc"].tobytes() == none["desc"].tobytes() and (same["src_idx"] == none["src_idx"]).all()


def test_greedy_triple_differs_from_all_earlier():
    a, b, c = (50, 60), (52, 60), (54.5, 60)
    assert X.near_merge(f32(a), f32(b), 3.0) and X.near_merge(f32(b), f32(c), 3.0) and not X.near_merge(f32(a), f32(c), 3.0)
    out = C.close(C.empty_rows(), C.rows_at([a, b, c]), pyramid(), CAP)
    assert out["refill"] == 1 and accepted(out).tolist() == [0, 2]           # all-earlier would reject C: B, itself rejected, is near it


def test_bound_at_exactly_the_distance():
    tracked = C.rows_at([(50, 60)])
    at = C.close(tracked, C.rows_at([(53, 64)]), pyramid(), CAP, min_dist=5.0)
    closer = C.close(tracked, C.rows_at([(np.nextafter(f32(53), f32(0)), 64)]), pyramid(), CAP, min_dist=5.0)
    assert accepted(at).tolist() == [0] and accepted(closer).tolist() == []


def test_nan_candidate_is_appended_and_dropped_by_the_description():
    cand = C.rows_at([(70, 60), (np.nan, np.nan), (90, 60)])
    out = C.close(C.rows_at([(50, 60)]), cand, pyramid(), CAP)
    assert accepted(out).tolist() == [0, 1, 2]
    assert sorted(out["src_idx"].tolist()) == [0, CAP, CAP + 2]


def test_levels_span_values_with_ties_and_the_order_is_stable():
    out = C.close(C.random_rows(60, 5), None, pyramid(), CAP)
    lev = out["level"][out["walk"]]
    values, counts = np.unique(lev, return_counts=True)
    assert len(values) >= 3 and (counts > 1).any() and (np.diff(lev) >= 0).all()
    for v in values:
        assert (np.diff(out["walk"][lev == v]) > 0).all()                    # ties keep their order
    assert (np.diff(out["walk"]) < 0).any()                                  # ... and the whole is a real reordering
    assert (out["octave"] != lev).any()                                      # the rows keep the DETECTION octave
    # an octave outside the level table: level -1, dropped; depth 0: level 0
    r = C.random_rows(4, 6)
    r["xy"][:] = r["xy_undist"][:] = [[60, 50], [80, 50], [100, 50], [120, 50]]
    r["octave"][:] = [100, -1, 8, 3]
    r["pts"][3] = 0
    o = C.close(r, None, pyramid(), CAP)
    assert o["level"][0] == -1 and o["level"][3] == 0 and sorted(o["src_idx"].tolist()) == [1, 2, 3]


def test_border_rows_are_dropped():
    xs = [np.nextafter(f32(31), f32(0)), 31, np.nextafter(f32(A.COLS - 31), f32(0)), A.COLS - 31]
    ys = [np.nextafter(f32(31), f32(0)), 31, np.nextafter(f32(A.ROWS - 31), f32(0)), A.ROWS - 31]
    pos = [(x, 60 + 5 * i) for i, x in enumerate(xs)] + [(70 + 5 * i, y) for i, y in enumerate(ys)] + [(30.99, 100)]
    out = C.close(C.rows_at(np.array(pos, f32) + 40, xy=pos), None, pyramid(), CAP)
    assert sorted(out["src_idx"].tolist()) == [1, 2, 5, 6] and out["walk"].tolist() == out["kept"].tolist()


def test_walk_differs_from_kept_only_for_a_dropped_row_within_its_tolerance_of_a_described_one():
    """:366 compares positions with a tolerance of 0.0001 px.  A row the description dropped that lies within it of the NEXT described
    row -- one ulp outside the border beside one inside, and earlier in the level order -- is taken in that row's place: the
    reference then pairs the dropped row's columns with the other row's descriptor.  The device follows keptIdx (each descriptor
    stays with its own row); everywhere else the two agree (the test below)."""
    inside, outside = np.nextafter(f32(A.ROWS - 31), f32(0)), f32(A.ROWS - 31)
    r = C.rows_at([(70, outside), (70, inside)])
    r["octave"][:] = 2
    r["det_dist"] = C.cur_dist(r["pts"])                                     # both at one level, the dropped row first
    out = C.close(r, None, pyramid(), CAP)
    assert out["level"][0] == out["level"][1] and out["kept"].tolist() == [1] and out["walk"].tolist() == [0]
    r2 = C.rows_at([(70, outside), (80, inside)])
    r2["octave"][:], r2["det_dist"] = 2, C.cur_dist(r2["pts"])
    out = C.close(r2, None, pyramid(), CAP)
    assert out["kept"].tolist() == [1] and out["walk"].tolist() == [1]


def test_seam_cases_cross_every_tile_seam_of_the_merge():
    """The cases of tests/test_gpu_track_close.py::test_merge_seams_*: 255 / 256 / 257 / 513 tracked rows (one, one, two and three
    trips of the tracked-row loop) against 513 and 1100 candidates (a third and a fifth tile).  With 1100: more than a tile of
    candidates is accepted before the last tile (the accepted-candidate loop takes a second trip); of the copies 512 .. 600 of
    candidates 0 .. 88 some are rejected though near no tracked row -- their original, accepted two tiles earlier, lies a pixel away
    -- and some are accepted because the original was itself rejected.  With 513: candidate 512 is a third tile of its own."""
    assert C.SEAM_CAP >= max(C.SEAM_TRACKED) and C.SEAM_CCAP >= max(C.SEAM_CANDIDATES) and C.SEAM_MINIMAL > max(C.SEAM_TRACKED)
    lo, hi = C.SEAM_COPIES
    for nt in C.SEAM_TRACKED:
        for nc in C.SEAM_CANDIDATES:
            tracked, cand = C.seam_case(nt, nc)
            assert len(tracked["xy"]) == nt and len(cand["xy"]) == nc
            copies = np.arange(lo, min(hi, nc))
            assert (cand["xy_undist"][copies] == cand["xy_undist"][copies - lo] + f32([1, 0])).all()
            s = C.merge_seams(tracked, cand, C.SEAM_MIN_DIST)
            acc = set(s["accepted"].tolist())
            out = C.close(tracked, cand, pyramid(), C.SEAM_CAP, C.SEAM_MINIMAL, C.SEAM_MIN_DIST)
            assert out["refill"] == 1 and accepted(out, C.SEAM_CAP).tolist() == s["accepted"].tolist()
            assert out["walk"].tolist() == out["kept"].tolist()
            if nc == 513:
                assert copies.tolist() == [512] and (nc - 1) // C.MERGE_TILE == 2
                continue
            rejected_by_original = [i for i in copies if i in s["earlier_only"] and i - lo in acc]
            accepted_after_rejected_original = [i for i in copies if i in acc and i - lo not in acc]
            print(nt, nc, "accepted", len(acc), "before the last tile", s["before_last"], "copies rejected by their original",
                  len(rejected_by_original), "copies accepted", len(accepted_after_rejected_original))
            assert len(rejected_by_original) > 0 and len(accepted_after_rejected_original) > 0
            assert s["before_last"] > C.MERGE_TILE and (nc - 1) // C.MERGE_TILE == 4
            assert len(s["second_trip_only"]) > 0      # rejected by an accepted candidate beyond the first 256 alone


def test_walk_of_the_reference_selects_the_kept_rows():
    for seed, n, m in ((11, 60, 0), (12, 20, 70), (13, 0, 30), (14, 63, 1)):
        tracked = C.random_rows(n, seed)
        cand = C.near_and_far_candidates(tracked, m, seed + 100) if m else None
        out = C.close(tracked, cand, pyramid(), CAP)
        assert out["walk"].tolist() == out["kept"].tolist() and len(out["desc"]) == len(out["walk"]), seed
        assert len(out["walk"]) < len(out["level"])                          # (the walk ran: rows were dropped)
