"""The two restatements of FAST-9/16 detection (tests/fast_ref.py) against each other and against hand-built cases, without a GPU:
the literal one (threshold table, early exits, consecutive-count loop, pairwise score, three row buffers, the grid loop with stable
sorts) and the closed form (arcs by min / max over rolled stacks, one lexicographic ordering)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fast_ref as F  # noqa: E402

SIZES = [(48, 64), (37, 53), (96, 128)]
THRESHOLDS = [0, 10, 40, 254, 255]


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0].dtype == b[0].dtype == np.float32


@pytest.mark.parametrize("scene", sorted(F.SCENES))
@pytest.mark.parametrize("rows,cols", SIZES)
def test_literal_equals_closed_form(scene, rows, cols):
    """Corner mask, score map and emitted list agree for every pixel of the three scenes at five thresholds, with and without
    suppression, on one image and through the grid loop."""
    img = F.SCENES[scene](rows, cols)
    for t in THRESHOLDS:
        corner, score, kps = F.fast_literal(img, t, True)
        c2, s2 = F.fast_closed(img, t)
        assert np.array_equal(corner, c2) and np.array_equal(score, s2), (scene, t)
        mask, resp = F.emitted_closed(c2, s2, True)
        y, x = np.nonzero(mask)
        assert kps == list(zip(x.tolist(), y.tolist(), resp[y, x].tolist())), (scene, t)
        corner0, score0, kps0 = F.fast_literal(img, t, False)
        assert np.array_equal(corner0, c2) and not score0.any()
        y, x = np.nonzero(c2)
        assert kps0 == [(a, b, 0) for a, b in zip(x.tolist(), y.tolist())]
        for nms, gr, gc, mx in [(True, 1, 1, 500), (True, 2, 3, 40), (False, 4, 4, 100), (True, 6, 4, 50), (False, 1, 1, 7)]:
            assert same(F.detect_literal(img, t, nms, gr, gc, mx), F.detect_closed(img, t, nms, gr, gc, mx)), (scene, t, nms, gr, gc, mx)


def test_scene_generators_give_the_figures_the_gpu_tests_rely_on():
    assert len(F.detect_closed(F.noise256(48, 64, 7), 10, True, 1, 1, 5000)[1]) == 268
    assert len(F.detect_closed(F.blocks(96, 128, 3, 120, noise=6), 10, True, 1, 1, 5000)[1]) == 253
    r = F.detect_closed(F.noise4(48, 64, 5), 10, True, 1, 1, 500)[1]
    assert r.tolist() == [119.0] * 24 + [59.0] * 87          # 111 key points, two responses: all but one cut fall inside a tie


def test_thresholds_outside_the_byte_range_are_clamped():
    img = F.SCENES["noise256"](37, 53)
    assert same(F.detect_closed(img, -5), F.detect_closed(img, 0)) and same(F.detect_literal(img, 300), F.detect_literal(img, 255))
    assert len(F.detect_closed(img, 255)[1]) == 0


def test_grey_conversion():
    rng = np.random.RandomState(2)
    img = rng.randint(0, 256, size=(31, 45, 3)).astype(np.uint8)
    img[0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 0, 255]]
    g = F.to_gray(img)
    c = img.astype(np.int64)
    assert np.array_equal(g, (c[..., 0] * 4899 + c[..., 1] * 9617 + c[..., 2] * 1868 + 8192) // 16384)
    assert g[0, :4].tolist() == [0, 255, 76, 29]
    real = 0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]
    assert np.abs(g.astype(np.float64) - real).max() <= 1.0
    assert not np.array_equal(g, F.to_gray(img[..., ::-1]))     # the weights are not symmetric: channel order matters
    assert F.to_gray(img[..., ::-1])[0, 2:4].tolist() == [29, 76]
    one = rng.randint(0, 256, size=(9, 9)).astype(np.uint8)
    assert np.array_equal(F.to_gray(one), one)                  # one channel: grey already


def ring_image(centre, ring_values, background=None):
    """A 7 x 7 image with `centre` at (3, 3) and ring_values[k] at ring position k."""
    img = np.full((7, 7), centre if background is None else background, np.uint8)
    img[3, 3] = centre
    for k, (dx, dy) in enumerate(F.RING):
        img[3 + dy, 3 + dx] = ring_values[k]
    return img


def both(img, t):
    """(corner, score) of the one candidate of a 7 x 7 image, from both restatements."""
    c1, s1, _ = F.fast_literal(img, t, True)
    c2, s2 = F.fast_closed(img, t)
    assert np.array_equal(c1, c2) and np.array_equal(s1, s2)
    assert c1.sum() == c1[3, 3] and s1.sum() == s1[3, 3]
    return int(c1[3, 3]), int(s1[3, 3])


def test_hand_built_arcs():
    t = 10
    arc = lambda start, n, inside, outside: [inside if (k - start) % 16 < n else outside for k in range(16)]   # noqa: E731
    # an arc of exactly nine darker pixels: d = 100 - 60 = 40 on the arc, 0 elsewhere -> corner, score 39
    assert both(ring_image(100, arc(2, 9, 60, 100)), t) == (1, 39)
    # eight are not enough
    assert both(ring_image(100, arc(2, 8, 60, 100)), t) == (0, 0)
    # an arc that wraps: positions 12 .. 4
    assert both(ring_image(100, arc(12, 9, 60, 100)), t) == (1, 39)
    assert both(ring_image(100, arc(12, 8, 60, 100)), t) == (0, 0)
    # the other polarity: nine brighter pixels, -d = 50
    assert both(ring_image(100, arc(5, 9, 150, 100)), t) == (1, 49)
    # the score is the LEAST difference of the best arc: nine of 60 with one of them only 85 -> d = 15
    ring = arc(0, 9, 60, 100)
    ring[4] = 85
    assert both(ring_image(100, ring), t) == (1, 14)
    # ten in a row of which the first is weaker: the arc without it scores higher
    ring = arc(0, 10, 60, 100)
    ring[0] = 85
    assert both(ring_image(100, ring), t) == (1, 39)
    # a difference of exactly t is not enough, t + 1 is: score max(t, t + 1) - 1 = t
    assert both(ring_image(100, arc(0, 9, 90, 100)), t) == (0, 0)
    assert both(ring_image(100, arc(0, 9, 89, 100)), t) == (1, 10)
    # the extremes: 255 over a ring of 0 scores 254; at t = 255 nothing is a corner; at t = 0 a difference of 1 scores 0
    assert both(ring_image(255, [0] * 16), t) == (1, 254)
    assert both(ring_image(255, [0] * 16), 254) == (1, 254)
    assert both(ring_image(255, [0] * 16), 255) == (0, 0)
    assert both(ring_image(0, [255] * 16), t) == (1, 254)
    assert both(ring_image(100, arc(3, 9, 99, 100)), 0) == (1, 0)
    # ... and such a corner of score 0 is never emitted under suppression, but is without
    img = ring_image(100, arc(3, 9, 99, 100))
    assert len(F.detect_closed(img, 0, True)[1]) == 0 and len(F.detect_literal(img, 0, True)[1]) == 0
    assert F.detect_closed(img, 0, False)[0].tolist() == [[3.0, 3.0]] and F.detect_literal(img, 0, False)[1].tolist() == [0.0]


def test_key_point_fields_of_a_single_corner():
    img = ring_image(200, [20] * 16, background=20)
    for fn in (F.detect_literal, F.detect_closed):
        xy, r = fn(img, 10, True, 1, 1, 5)
        assert xy.tolist() == [[3.0, 3.0]] and r.tolist() == [179.0] and xy.dtype == np.float32 and r.dtype == np.float32


def test_two_adjacent_equal_scores_emit_neither():
    """Two bright pixels side by side on a dark ground: both are corners with the same score, each suppresses the other; one
    alone is emitted."""
    img = np.full((9, 10), 20, np.uint8)
    img[4, 4] = img[4, 5] = 200
    c, s = F.fast_closed(img, 10)
    assert c[4, 4] == 1 and c[4, 5] == 1 and s[4, 4] == s[4, 5] > 0
    assert len(F.detect_closed(img, 10, True)[1]) == 0 and len(F.detect_literal(img, 10, True)[1]) == 0
    assert len(F.detect_closed(img, 10, False)[1]) == int(c.sum()) >= 2
    img[4, 5] = 20
    assert F.detect_closed(img, 10, True)[0].tolist() == [[4.0, 4.0]] and F.detect_literal(img, 10, True)[0].tolist() == [[4.0, 4.0]]
    # a strictly larger neighbour wins alone
    img[4, 5] = 180
    img[4, 4] = 220
    xy = F.detect_closed(img, 10, True)[0]
    assert [4.0, 4.0] in xy.tolist() and [5.0, 4.0] not in xy.tolist() and same(F.detect_closed(img, 10, True), F.detect_literal(img, 10, True))


def test_sizes_without_a_candidate():
    for rows, cols in [(6, 9), (9, 6), (1, 1), (3, 40)]:
        img = F.noise256(rows, cols, 4)
        for fn in (F.detect_literal, F.detect_closed):
            assert len(fn(img, 0, False)[1]) == 0
    img = np.zeros((7, 7), np.uint8)
    img[3, 3] = 90
    c, s = F.fast_closed(img, 10)
    assert c.sum() == 1 and c[3, 3] == 1 and s[3, 3] == 89
    full = F.noise256(7, 7, 4)
    assert F.fast_literal(full, 0, False)[0][np.arange(7) != 3].sum() == 0      # only (3, 3) can be a corner


def test_grid_geometry():
    # 53 x 37 (cols x rows) at 3 x 2 (gridCols x gridRows): ROIs of 17 x 18; the columns' origins are 0, 17, 35 -- column 34 and
    # column 52 belong to no ROI, and row 36 to none
    assert F.roi_rects(37, 53, 2, 3) == [(0, 0, 17, 18), (0, 18, 17, 18), (17, 0, 17, 18), (17, 18, 17, 18), (35, 0, 17, 18), (35, 18, 17, 18)]
    # 4 x 6: ROIs of 13 x 6, too low for a candidate
    rects = F.roi_rects(37, 53, 6, 4)
    assert len(rects) == 24 and all(r[2:] == (13, 6) for r in rects) and rects[1] == (0, 6, 13, 6) and rects[6] == (13, 0, 13, 6)
    img = F.noise256(37, 53, 7)
    for fn in (F.detect_literal, F.detect_closed):
        assert len(fn(img, 10, True, 6, 4, 500)[1]) == 0
    # a pixel outside every ROI is never a key point: columns 34 and 52 and row 36 at 3 x 2
    _, score, corner = F.maps_closed(img, 10, 2, 3)
    assert not corner[:, 34].any() and not corner[:, 52].any() and not corner[36].any() and corner.any()
    assert not corner[:, 17:20].any() and not corner[:, 14:17].any() and not corner[15:21].any()     # the ROIs' own margins
    assert F.max_in_roi(500, 1, 1) == 1500 and F.max_in_roi(500, 4, 4) == 93 and F.max_in_roi(20, 2, 3) == 10


def test_corner_straddling_an_roi_edge():
    """A corner whose ring crosses the line between two ROIs is found with grid 1 x 1 and lost with 2 x 1."""
    img = np.full((20, 40), 30, np.uint8)
    img[10, 20] = 220            # columns 20 .. 39 are the second ROI of two: the pixel sits on its column 0
    for fn in (F.detect_literal, F.detect_closed):
        assert fn(img, 10, True, 1, 1, 50)[0].tolist() == [[20.0, 10.0]]
        assert len(fn(img, 10, True, 1, 2, 50)[1]) == 0
    img2 = np.full((20, 40), 30, np.uint8)
    img2[10, 23] = 220           # three columns in: a candidate of the second ROI, reported in image coordinates
    for fn in (F.detect_literal, F.detect_closed):
        assert fn(img2, 10, True, 1, 2, 50)[0].tolist() == [[23.0, 10.0]]


def test_max_in_roi_zero():
    """maxInROI = max * 3 / (gridCols * gridRows) in integer arithmetic: 0 when 3 max < the number of ROIs."""
    img = F.SCENES["noise256"](48, 64)
    assert F.max_in_roi(2, 3, 3) == 0 and F.max_in_roi(3, 3, 3) == 1
    for fn in (F.detect_literal, F.detect_closed):
        assert len(fn(img, 10, True, 3, 3, 2)[1]) == 0
        assert len(fn(img, 10, True, 3, 3, 3)[1]) == 3
        assert len(fn(img, 10, True, 1, 1, 0)[1]) == 0


def test_orderings_are_stable():
    """Among equal responses: raster order inside an ROI, the ROI loop's order (columns outer, rows inner) across ROIs."""
    img = F.noise4(48, 64, 5)
    xy, r = F.detect_closed(img, 10, True, 1, 1, 500)
    for v in np.unique(r):
        p = xy[r == v]
        key = p[:, 1].astype(np.int64) * 64 + p[:, 0].astype(np.int64)
        assert (np.diff(key) > 0).all()
    xy, r = F.detect_closed(img, 10, True, 2, 2, 500)
    roi = (xy[:, 0] >= 32).astype(np.int64) * 2 + (xy[:, 1] >= 24).astype(np.int64)      # k * gridRows + i
    for v in np.unique(r):
        assert (np.diff(roi[r == v]) >= 0).all()
    assert (np.diff(r) <= 0).all()
