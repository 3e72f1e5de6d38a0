"""The sequential restatement of the Lucas-Kanade tracker (tests/klt_ref.py) checked on the host: its integer passes against an
independent scipy computation, its behaviour on scenes whose answer is known, its exits, and its selection pair by pair against
the vectorised form.  No GPU: this is the yardstick's own test."""
import numpy as np
import pytest

import klt_ref as K


@pytest.mark.parametrize("rows,cols,cn", [(48, 64, 1), (37, 53, 3), (9, 8, 1)])
def test_pyramid_and_scharr_equal_an_independent_correlation(rows, cols, cn):
    import scipy.ndimage as scipy_ndimage
    rng = np.random.default_rng(rows * 100 + cols)
    img = rng.integers(0, 256, (rows, cols, cn), dtype=np.uint8)
    k1 = np.array([1, 4, 6, 4, 1], np.int64)
    sx = np.array([[-3, 0, 3], [-10, 0, 10], [-3, 0, 3]], np.int64)
    for c in range(cn):
        plane = img[:, :, c].astype(np.int64)
        full = scipy_ndimage.correlate(plane, np.outer(k1, k1), mode="mirror")
        assert np.array_equal(K.pyr_down(img)[:, :, c], ((full[::2, ::2] + 128) >> 8).astype(np.uint8))
        d = K.scharr(img)
        assert d.dtype == np.int16
        assert np.array_equal(d[:, :, c, 0], scipy_ndimage.correlate(plane, sx, mode="mirror"))
        assert np.array_equal(d[:, :, c, 1], scipy_ndimage.correlate(plane, sx.T, mode="mirror"))
    assert K.pyr_down(img).shape == ((rows + 1) // 2, (cols + 1) // 2, cn)


def test_level_count_and_borders():
    assert K.level_count(48, 64, 7, 3) == 2        # 24 x 32, 12 x 16, then 6 x 8: not built
    assert K.level_count(37, 53, 7, 3) == 2        # 19 x 27, 10 x 14, then 5 x 7
    assert K.level_count(96, 128, 7, 3) == 3
    assert K.level_count(64, 80, 21, 3) == 1
    assert K.level_count(48, 64, 7, 0) == 0
    with pytest.raises(ValueError):
        K.build_pyramid(np.zeros((7, 40), np.uint8), 7, 3)
    img = np.arange(5 * 6, dtype=np.uint8).reshape(5, 6, 1)
    pad = K.pad_image(img, 3)
    assert pad.shape == (11, 12, 1) and pad[3, 0, 0] == img[0, 3, 0] and pad[0, 3, 0] == img[3, 0, 0] and pad[10, 11, 0] == img[1, 2, 0]
    assert not K.pad_deriv(K.scharr(img), 3)[:3].any()
    assert K.clamp_params(150, 20.0) == (100, 100.0) and K.clamp_params(-3, -1.0) == (0, 0.0)


def test_identical_pair_stays_put_with_zero_error():
    img = K.smooth_texture(48, 64, 1, seed=4)
    rng = np.random.default_rng(1)
    pts = np.stack([rng.uniform(8, 55, 40), rng.uniform(8, 39, 40)], 1).astype(np.float32)
    nxt, status, err = K.track(img, img, pts, 7, 3, 30, 0.01)
    assert status.all() and not err.any()
    assert np.abs(nxt - pts).max() < 1e-4          # ((p - half) + half need not round-trip)


def test_constant_image_fails_every_point():
    img = np.full((48, 64), 90, np.uint8)
    pts = K.random_points(48, 64, 30, 2)
    _, status, err = K.track(img, img, pts, 7, 3, 30, 0.01)
    assert not status.any() and not err.any()
    _, status, err = K.track(img, img, pts, 7, 3, 30, 0.01, flags=K.GET_MIN_EIGENVALS)
    assert not status.any() and not err.any()      # (the smaller eigenvalue of a zero matrix)


# (rows, cols, window, true shift, twice the worst interior error measured below)
KNOWN_FLOW = [(48, 64, 7, (1.3, -0.7), 0.110), (37, 53, 7, (3.6, 2.2), 0.069), (96, 128, 7, (5.4, -3.1), 0.132),
              (64, 80, 21, (2.5, 1.5), 0.034)]


@pytest.mark.parametrize("rows,cols,win,shift,bound", KNOWN_FLOW)
def test_known_flow_is_recovered(rows, cols, win, shift, bound):
    """A smooth analytic texture sampled at shifted coordinates: the recovered flow of interior status-1 points against the true
    shift, maxLevels 3, 30 iterations, eps 0.01, 80 random points.  Measured with this restatement (interior = further than
    win + 2 + |shift| from every edge):

        scene (rows x cols)   shift (px)     interior points   worst error (px)   median (px)
        48 x 64               (1.3, -0.7)    33                0.0548             0.0206
        37 x 53               (3.6, 2.2)     15                0.0341             0.0123
        96 x 128              (5.4, -3.1)    46                0.0658             0.0148
        64 x 80, window 21    (2.5, 1.5)     5                 0.0169             0.0058

    The bound is twice the measured worst error: the mistakes this guards against (sign of delta, level scaling, half-window
    offset) cost whole pixels."""
    a = K.smooth_texture(rows, cols, 1, seed=11)
    b = K.smooth_texture(rows, cols, 1, seed=11, shift=(-shift[0], -shift[1]))
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(0, cols - 1, 80), rng.uniform(0, rows - 1, 80)], 1).astype(np.float32)
    nxt, status, _ = K.track(a, b, pts, win, 3, 30, 0.01)
    m = win + 2 + max(abs(shift[0]), abs(shift[1]))
    interior = (pts[:, 0] > m) & (pts[:, 0] < cols - 1 - m) & (pts[:, 1] > m) & (pts[:, 1] < rows - 1 - m) & (status == 1)
    assert interior.sum() >= 5
    e = np.hypot(nxt[:, 0] - pts[:, 0] - shift[0], nxt[:, 1] - pts[:, 1] - shift[1])[interior]
    print("worst %.4f median %.4f over %d interior points" % (e.max(), np.median(e), interior.sum()))
    assert e.max() <= bound


def test_main_scene_takes_every_exit():
    """The GPU test's main scene (klt_ref.main_scene) ends (point, level) walks at every exit of the tracker: the minEig / D
    gate, outside before iterating, outside while iterating, the eps break, the oscillation break and the iteration cap."""
    prev, nxt, pts = K.main_scene()
    m, exits = K.MAIN_SCENE, {}
    K.track(prev, nxt, pts, m["win"], m["max_levels"], m["max_count"], m["eps"], exits=exits)
    print(exits)
    assert set(exits) == set(K.EXITS) and all(v > 0 for v in exits.values()), exits
    assert sum(exits.values()) == len(pts) * (K.level_count(m["rows"], m["cols"], m["win"], m["max_levels"]) + 1)


@pytest.mark.parametrize("case", K.selection_lists(), ids=lambda c: c[0])
def test_selection_pairwise_equals_vectorised(case):
    _, pts, status, err, thr, dist = case
    kept_a, m_a = K.select_pairwise(pts, status, err, thr, dist)
    kept_b, m_b = K.select_vectorised(pts, status, err, thr, dist)
    assert np.array_equal(kept_a, kept_b) and np.array_equal(m_a, m_b)


def test_selection_known_answers():
    lists = {c[0]: c for c in K.selection_lists()}
    kept = lambda name: K.select_pairwise(*lists[name][1:])[0].tolist()   # noqa: E731
    assert kept("equal errors: the later index goes") == [0, 3]
    assert kept("failed points still knock out neighbours") == []        # 1 loses to failed 0, 2 to failed 3, 4 fails the gate
    assert kept("exact distance is not below it") == [0, 1]               # |p0 - p1| = 5 is not < 5; 2 is near both and worse
    assert kept("zero distance: nothing is near") == [0, 1]
