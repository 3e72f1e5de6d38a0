"""The two restatements of ORB description (tests/orb_ref.py) against each other and against known answers, without a GPU: the
literal one with scalar loops and the vectorised one, on every scene, shape and key-point set the device tests use."""
import hashlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import orb_ref as R  # noqa: E402

SHAPES = [(9, 13), (37, 53), (63, 64), (80, 96)]


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("cn", [1, 3])
def test_planes_literal_equals_vectorised(rows, cols, cn):
    for i, name in enumerate(R.SCENES):
        img = R.scene(name, rows, cols, cn, seed=i)
        for sf, nl in ((1.2, 8), (1.5, 6)):
            if (sf, nl) != (1.2, 8) and name != "noise":
                continue
            a, b = R.pyramid(img, sf, nl), R.pyramid(img, sf, nl, loops=True)
            assert len(a) == len(b) == nl
            for (r1, b1, s1), (r2, b2, s2) in zip(a, b):
                assert r1.tobytes() == r2.tobytes() and b1.tobytes() == b2.tobytes() and s1 == s2 and r1.shape == r2.shape


def test_level_sizes_at_vga():
    got = [(r, c) for r, c, _ in R.level_geometry(480, 640, 1.2, 8)]
    assert got == [(480, 640), (400, 533), (333, 444), (278, 370), (231, 309), (193, 257), (161, 214), (134, 179)]
    assert R.level_geometry(9, 13, 1.2, 8)[-1][:2] == (3, 4)
    assert R.level_geometry(480, 640)[0][2] == np.float32(1) and R.level_geometry(480, 640)[1][2] == np.float32(1.2)


def test_constants_through_resize_and_blur():
    for raw, blr, _ in R.pyramid(np.full((37, 53), 255, np.uint8)):
        assert (raw == 255).all() and (blr == 255).all()
    for raw, blr, _ in R.pyramid(np.full((37, 53, 3), 128, np.uint8)):
        assert (raw == 128).all() and (blr == 129).all()   # the taps sum to 257


def test_coefficient_pairs_sum_to_2048():
    for sn, dn in ((640, 533), (533, 444), (13, 11), (4, 3), (64, 43), (2, 1)):
        for columns in (True, False):
            s0, s1, a0, a1 = R.resize_coeffs(sn, dn, columns)
            assert ((a0 + a1) == 2048).all() and (a0 >= 0).all() and (a1 >= 0).all()
            assert (s0 >= 0).all() and (s1 <= sn - 1).all() and ((s1 - s0) >= 0).all() and ((s1 - s0) <= 1).all()


def test_default_pattern():
    p = R.default_pattern()
    assert p.dtype == np.int8 and p.shape == (256, 4) and p.min() >= -15 and p.max() <= 15
    assert p[:4].tolist() == [[11, -7, -5, -7], [-7, 0, -2, -1], [-8, -3, 5, -8], [-8, 0, -12, -6]]
    assert not ((p[:, 0] == p[:, 2]) & (p[:, 1] == p[:, 3])).any()
    assert hashlib.sha256(p.tobytes()).hexdigest() == "07c6577a48e06e09d7accbca60a6475e40dcfc260f662a9f9b1350303fc8d9c9"
    reach = np.sqrt((p.astype(np.float64) ** 2).reshape(512, 2).sum(axis=1)).max()
    assert reach < 22.0   # inside the 32-pixel border of OpenCV's atlas


def test_rotation_bar():
    """absolute error against float64 cos / sin at most 2^-20 over -360 .. 720 in steps of 1/64, plus -1"""
    ang = np.concatenate([np.arange(-360 * 64, 720 * 64 + 1) / 64.0, [-1.0]]).astype(np.float32)
    a, b = R.rotation(ang)
    rad = np.deg2rad(ang.astype(np.float64))
    err = max(np.abs(a - np.cos(rad)).max(), np.abs(b - np.sin(rad)).max())
    print("worst rotation error %.3e = %.4f x 2^-20" % (err, err * 2 ** 20))
    assert err <= 2.0 ** -20
    for i in list(range(0, len(ang), 1009)) + [len(ang) - 1]:
        la, lb = R.rotation_loops(ang[i])
        assert la.tobytes() == a[i].tobytes() and lb.tobytes() == b[i].tobytes()
    for bad in (np.nan, np.inf, -np.inf, 3e6):
        assert R.rotation_loops(np.float32(bad)) == R.rotation_loops(np.float32(0)) == (np.float32(1), np.float32(0))
        assert tuple(float(v) for v in R.rotation(np.float32(bad))) == (1.0, 0.0)


def both(pyr, xy, angle, octave, pattern=None, counters=None):
    d1, k1 = R.describe_loops(pyr, xy, angle, octave, pattern, counters)
    seen = None if counters is None else R.new_counters()
    d2, k2 = R.describe(pyr, xy, angle, octave, pattern, seen)
    if counters is not None:   # the vectorised form counts what the loops count (every caller passes new_counters())
        assert seen == counters, (seen, counters)
    assert d1.tobytes() == d2.tobytes() and k1.tobytes() == k2.tobytes() and k1.dtype == k2.dtype == np.int32
    return d1, k1


def test_rows_random_set_meets_its_conditions():
    pyr = R.pyramid(R.texture(80, 96, 3))
    xy, angle, octave = R.random_keypoints(64, 80, 96, 8, seed=5)
    cnt = R.new_counters()
    desc, kept = both(pyr, xy, angle, octave, counters=cnt)
    print(cnt)
    assert len(kept) == 64 and cnt["samples"] == 64 * 512
    assert cnt["outside"] > 0 and cnt["reach"] <= 32
    assert len(set(bytes(r) for r in desc)) == 64
    assert (np.diff(octave[kept]) >= 0).all()
    for l in range(8):   # stable inside an octave
        assert (np.diff(kept[octave[kept] == l]) > 0).all()


def test_rows_edges_and_custom_pattern():
    pyr = R.pyramid(R.texture(80, 96, 3))
    xy, angle, octave = R.edge_keypoints(80, 96, 8)
    desc, kept = both(pyr, xy, angle, octave)
    dropped = sorted(set(range(len(octave))) - set(kept.tolist()))
    assert dropped == [1, 2, 4, 6, 7, 9, 10, 11]   # below 31, at cols - 31 / rows - 31, NaN, octaves -1 and 8
    pat = R.corner_pattern()
    d2, k2 = both(pyr, xy, angle, octave, pat)
    assert k2.tobytes() == kept.tobytes() and not (d2[:, 0] & 2).any() and d2.tobytes() != desc.tobytes()
    none, nk = both(pyr, xy[:0], angle[:0], octave[:0])
    assert none.shape == (0, 32) and nk.shape == (0,)
    zero, zk = both(pyr, xy, angle, np.zeros_like(octave))
    assert zk.tolist() == [i for i in range(len(octave)) if i not in (1, 2, 4, 6, 7, 9)]


def test_rows_bounce_more_than_once_on_a_small_pyramid():
    pyr = R.pyramid(R.texture(63, 64, 9), 1.5, 6)
    assert pyr[5][0].shape == (8, 8)
    xy = np.array([[31, 31], [32.5, 31.5], [32.99, 31.99]] * 6, np.float32)
    angle = np.linspace(0, 350, 18).astype(np.float32)
    octave = np.repeat(np.arange(6), 3).astype(np.int32)[::-1].copy()
    cnt = R.new_counters()
    desc, kept = both(pyr, xy, angle, octave, counters=cnt)
    print(cnt)
    assert len(kept) == 18 and cnt["bounced"] > 0 and cnt["reach"] <= 32
    assert both(R.pyramid(R.texture(62, 96, 1)), [[40, 31]], [0], [0])[1].shape == (0,)   # rows <= 62: nothing is kept
