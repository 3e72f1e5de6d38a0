"""The two restatements of ORB detection (tests/orb_detect_ref.py) against each other and against the
hand-checked pieces of the reading -- no GPU.  The premises of the device tests are asserted here, on the restatement, so that a
device test cannot pass by never cutting."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orb_detect_ref as D  # noqa: E402

f32 = np.float32


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_quota_vectors():
    assert D.quotas(500, 1.2, 8) == [109, 90, 75, 63, 52, 44, 36, 31]
    assert D.quotas(500, 1.2, 3) == [198, 165, 137]
    assert D.quotas(40, 1.2, 4) == [13, 11, 9, 7]
    assert D.quotas(2, 1.2, 3) == [1, 1, 0] and D.quotas(0, 1.2, 8) == [0] * 8 and D.quotas(33, 1.2, 1) == [33]


def test_umax_table_comes_out_of_the_construction():
    assert D.umax_construction() == D.UMAX == (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)
    assert int(D._DISC.sum()) == sum(2 * u + 1 for u in D.UMAX) * 2 - 31 == len(D.DISC_DU)


def test_fast_atan2_meets_the_documented_bar():
    """0.3 degrees against float64 atan2 on the circle (OpenCV's documented accuracy); measured over these vectors: 0.0096."""
    rng = np.random.RandomState(1)
    v = rng.randint(-200000, 200001, size=(2000000, 2))
    v = v[(v != 0).any(axis=1)]
    got = D.fast_atan2_v(v[:, 1].astype(f32), v[:, 0].astype(f32)).astype(np.float64)
    want = np.degrees(np.arctan2(v[:, 1].astype(f32).astype(np.float64), v[:, 0].astype(f32).astype(np.float64))) % 360.0
    err = np.abs(got - want)
    err = np.minimum(err, 360.0 - err)
    print("fastAtan2 worst error, degrees:", err.max())
    assert err.max() <= 0.3
    assert 0.0 <= got.min() and got.max() <= 360.0
    idx = rng.randint(0, len(v), 300)
    assert [D.fast_atan2(v[i, 1], v[i, 0]).tobytes() for i in idx] == [D.fast_atan2_v(f32(v[i, 1]), f32(v[i, 0])).tobytes() for i in idx]


def test_fast_atan2_on_the_axes_and_at_the_origin():
    for (y, x), want in [((0, 0), 0.0), ((0, 5), 0.0), ((7, 0), 90.0), ((0, -3), 180.0), ((-2, 0), 270.0)]:
        assert float(D.fast_atan2(y, x)) == want == float(D.fast_atan2_v(f32(y), f32(x))), (y, x)
    assert abs(float(D.fast_atan2(1, 1)) - 45.0) < 0.01 and abs(float(D.fast_atan2(-1, -1)) - 225.0) < 0.01


def test_harris_of_named_patches():
    flat = np.full((11, 11), 93, np.uint8)
    assert D.harris_sums_literal(flat, 5, 5) == (0, 0, 0) and float(D.harris_response(0, 0, 0)) == 0.0
    edge = np.zeros((11, 11), np.uint8)
    edge[:, 6:] = 10     # a step between columns 5 and 6: Ix = 40 in columns 5 and 6 of the block's seven rows
    assert D.harris_sums_literal(edge, 5, 5) == (14 * 1600, 0, 0)
    assert float(D.harris_response(14 * 1600, 0, 0)) < 0.0
    corner = np.zeros((11, 11), np.uint8)
    corner[6:, 6:] = 10  # a quadrant: in columns 5 and 6 Ix is 10, 30, 40, 40 over rows 5 .. 8, Iy the transpose; c = (10 + 30)^2
    assert D.harris_sums_literal(corner, 5, 5) == (8400, 8400, 1600)
    for img, want in ((flat, (0, 0, 0)), (edge, (22400, 0, 0)), (corner, (8400, 8400, 1600))):
        assert tuple(int(m[5, 5]) for m in D.harris_maps(img)) == want
    r = D.harris_response(8400, 8400, 1600)
    assert r.dtype == f32 and float(r) > 0.0
    # the float sequence, operation by operation
    s = f32(1) / f32(7140)
    s4 = f32(f32(f32(s * s) * s) * s)
    fa, fc = f32(8400), f32(1600)
    want = f32(f32(f32(fa * fa) - f32(fc * fc)) - f32(f32(f32(0.04) * f32(fa + fa)) * f32(fa + fa))) * s4
    assert r.tobytes() == f32(want).tobytes()


def test_retain_best_keeps_every_tie():
    kps = [(i, v) for i, v in enumerate([5, 9, 5, 7, 5, 1, 9])]
    key = lambda k: k[1]  # noqa: E731
    assert D.retain_best_literal(kps, 0, key) == []
    assert D.retain_best_literal(kps, 7, key) == kps and D.retain_best_literal(kps, 9, key) == kps
    assert [k[0] for k in D.retain_best_literal(kps, 1, key)] == [1, 6]
    assert [k[0] for k in D.retain_best_literal(kps, 3, key)] == [1, 3, 6]
    assert [k[0] for k in D.retain_best_literal(kps, 4, key)] == [0, 1, 2, 3, 4, 6]


def live(lv):
    return lv["raw"].shape[0] > 2 * D.EDGE and lv["raw"].shape[1] > 2 * D.EDGE


@pytest.mark.parametrize("case", D.PREMISE_CASES, ids=lambda c: "%s-%dx%d-%d" % c[:4])
def test_premises_of_the_device_tests(case):
    """At every live level both cuts bite; in at least one level a tie at the first cut makes the survivors exceed 2 q_l."""
    name, rows, cols, cn, p = case
    levels = D.detect_closed(D.image(name, rows, cols, cn), p, want_levels=True)[4][0]
    lives = [lv for lv in levels if live(lv)]
    assert len(lives) == (3 if rows == 96 else 5) and all(live(lv) for lv in levels[:len(lives)])
    for lv in lives:
        assert lv["quota"] > 0 and lv["candidates"] > 2 * lv["quota"], (lv["candidates"], lv["quota"])
        assert len(lv["x"]) > lv["quota"] and int(lv["kept"].sum()) < len(lv["x"])
    assert any(len(lv["x"]) > 2 * lv["quota"] for lv in lives)


def test_level_shapes_of_the_named_sizes():
    import orb_ref as O
    assert [(r, c) for r, c, _ in O.level_geometry(96, 128, 1.2, 4)] == [(96, 128), (80, 107), (67, 89), (56, 74)]
    g = O.level_geometry(150, 200, 1.2, 8)
    assert [r > 62 and c > 62 for r, c, _ in g] == [True] * 5 + [False] * 3


def test_colour_scene_separates_the_two_grey_conversions():
    import fast_ref as F
    import orb_ref as O
    img = D.image("noise256", 96, 128, 3)
    assert not np.array_equal(F.to_gray(img), O.gray(img))
    p = D.PREMISE_CASES[1][4]
    assert not same(D.detect_closed(img, p), D.detect_closed(img[..., ::-1], p))


def test_tiled_scene_ties_straddle_both_cuts():
    name, rows, cols, cn, p = D.TILED_CASE
    img = D.image(name, rows, cols, cn)
    xy, resp, ang, octv, levels = D.detect_closed(img, p, want_levels=True)
    lv = levels[0][0]
    r = np.sort(lv["response"].view(np.uint32))[::-1]   # (positive floats: their words order like they do)
    assert (lv["response"] > 0).all()
    q = lv["quota"]
    assert q == 5 and len(r) > q and r[q - 1] == r[q] and int(lv["kept"].sum()) == 8 > q      # the second cut falls inside a tie
    top = resp.view(np.uint32)
    assert (top[:8] == top[0]).all() and top[8] != top[0] and octv[:8].tolist() == [0] * 8     # ... and so does every final cut 1 .. 7
    # the tied block comes out in raster order
    yx = [(float(y), float(x)) for x, y in xy[:8]]
    assert yx == sorted(yx)


@pytest.mark.parametrize("case", D.ALL_CASES, ids=lambda c: "%s-%dx%d-%d-%s" % (c[:4] + ("-".join(str(v) for v in c[4].values()),)))
def test_literal_equals_closed_form(case):
    name, rows, cols, cn, p = case
    img = D.image(name, rows, cols, cn)
    a, b = D.detect_literal(img, p), D.detect_closed(img, p)
    assert same(a, b), (len(a[1]), len(b[1]))
    if p["n_features"] == 0 or rows == 62:
        assert len(b[1]) == 0


def test_edge_shapes():
    big = D.detect_closed(D.image("noise256", 63, 64), D.params(20, 1.2, 8), want_levels=True)
    assert all(0 <= len(lv["x"]) <= 2 for lv in big[4][0]) and not any(live(lv) for lv in big[4][0][1:])
    assert len(D.detect_closed(D.image("noise256", 62, 90), D.params(20, 1.2, 8))[1]) == 0


def test_max_features_cuts_through_the_tied_block():
    name, rows, cols, cn, p = D.TILED_CASE
    img = D.image(name, rows, cols, cn)
    full = D.detect_closed(img, p)
    for mx in range(0, 10):
        q = dict(p, max_features=mx)
        a, b = D.detect_literal(img, q), D.detect_closed(img, q)
        assert same(a, b) and len(b[1]) == mx
        assert same(b, tuple(v[:mx] for v in full))     # (3 mx per ROI never bites before mx does at 1 x 1)
