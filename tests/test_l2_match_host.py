"""The float-descriptor matcher's definition (tests/l2_match_ref.py) checked on the host: against a float64 brute force, on known
answers, on the order of its tail sums; the ABI mirror's size; the argument rejections that need no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import l2_match_ref as ref  # noqa: E402

f32 = np.float32


def _scalar_l2sqr(a, b):
    """The definition once more, one float32 scalar operation at a time."""
    a = [f32(x) for x in a]
    b = [f32(x) for x in b]
    D, j, d = len(a), 0, f32(0)
    if D >= 8:
        acc0, acc1 = [f32(0)] * 4, [f32(0)] * 4
        while j <= D - 8:
            for i in range(4):
                t0, t1 = f32(a[j + i] - b[j + i]), f32(a[j + 4 + i] - b[j + 4 + i])
                acc0[i] = f32(acc0[i] + f32(t0 * t0))
                acc1[i] = f32(acc1[i] + f32(t1 * t1))
            j += 8
        s = [f32(acc0[i] + acc1[i]) for i in range(4)]
        d = f32(f32(f32(s[0] + s[1]) + s[2]) + s[3])
    while j <= D - 4:
        t = [f32(a[j + i] - b[j + i]) for i in range(4)]
        d = f32(d + f32(f32(f32(f32(t[0] * t[0]) + f32(t[1] * t[1])) + f32(t[2] * t[2])) + f32(t[3] * t[3])))
        j += 4
    while j < D:
        t = f32(a[j] - b[j])
        d = f32(d + f32(t * t))
        j += 1
    return d


@pytest.mark.parametrize("D", [1, 3, 4, 7, 8, 9, 12, 13, 64, 65])
def test_tail_order(D):
    rng = np.random.default_rng(100 + D)
    a = (rng.standard_normal((6, D)) * 3).astype(f32)
    b = (rng.standard_normal((5, D)) * 3).astype(f32)
    m = ref.l2sqr_matrix(a, b)
    for i in range(6):
        for k in range(5):
            assert m[i, k].tobytes() == _scalar_l2sqr(a[i], b[k]).tobytes(), (D, i, k)


def test_tail_order_is_not_a_plain_running_sum():
    """D = 12: one block of eight (lane accumulators) and one block of four added as ((t0 + t1) + t2) + t3 -- on data where a
    running sum over the twelve squares rounds differently."""
    found = 0
    rng = np.random.default_rng(5)
    for _ in range(200):
        a = (rng.standard_normal(12) * 100).astype(f32)
        b = (rng.standard_normal(12) * 100).astype(f32)
        run = f32(0)
        for j in range(12):
            t = f32(a[j] - b[j])
            run = f32(run + f32(t * t))
        found += run.tobytes() != ref.l2sqr(a, b).tobytes()
    assert found > 20


@pytest.mark.parametrize("scene", ["surf", "sift"])
def test_restatement_against_float64_brute_force(scene):
    q, t = (ref.surf_scene if scene == "surf" else ref.sift_scene)(301, 297, index=3)
    m = ref.match_l2(q, t)
    want = ref.match_l2_f64(q, t)
    assert len(m) == len(want) and len(m) > 150
    assert [(int(x["queryIdx"]), int(x["trainIdx"])) for x in m] == [(a, b) for a, b, _ in want]
    d64 = np.array([w[2] for w in want])
    assert np.all(np.abs(m["distance"] - d64) <= 4e-6 * np.maximum(d64, 1e-30)) and np.all(m["imgIdx"] == 0)


def test_known_answers():
    e = np.eye(8, dtype=f32)
    # identical rows: distance 0
    m = ref.match_l2(e[:3], e[:3])
    assert m["queryIdx"].tolist() == [0, 1, 2] and m["trainIdx"].tolist() == [0, 1, 2] and m["distance"].tolist() == [0, 0, 0]
    # step 1 ties to the lowest query, step 2 ties to the lowest train row; a query nobody chose is omitted
    q = np.stack([e[0], e[0], e[1]])            # queries 0 and 1 identical, query 2 apart
    t = np.stack([e[0], e[0], e[2]])            # trains 0 and 1 identical (both choose query 0), train 2 equidistant to all
    m = ref.match_l2(q, t)
    assert [(int(x["queryIdx"]), int(x["trainIdx"])) for x in m] == [(0, 0)]
    assert m["distance"][0] == 0
    # a train row that is all NaN chooses nobody; +inf distances are never chosen
    t2 = np.stack([np.full(8, np.nan, f32), e[1], np.full(8, 3e38, f32)])
    m = ref.match_l2(q, t2)
    assert [(int(x["queryIdx"]), int(x["trainIdx"])) for x in m] == [(2, 1)]
    # either side empty
    assert len(ref.match_l2(q[:0], t)) == 0 and len(ref.match_l2(q, t[:0])) == 0


def test_square_roots_tie_where_sums_differ():
    """About half of all adjacent float sums share a square root: comparisons are made on the roots."""
    x = np.linspace(1.0, 2.0, 4001).astype(f32)
    nxt = np.nextafter(x, f32(4))
    assert 0.3 < np.mean(np.sqrt(x) == np.sqrt(nxt)) < 0.7


def test_struct_size_and_rejections_without_a_device():
    from putslam_amd import _abi, _lib
    L = _lib.load()
    assert _lib.struct_sizes_f32() == {"frameset_f32": 64} and L.ps_abi_sizeof_frameset_f32() == 64
    assert C.sizeof(_abi.PsFrameSetF32) == 64 and _abi.PS_MAX_L2_DIM == 512
    n = C.c_int(7)
    out = np.zeros(4, _abi.DMATCH_DTYPE)
    assert L.ps_match_l2_f32(None, None, 0, 0, None, 0, 0, 64, out.ctypes.data_as(C.c_void_p), C.byref(n)) == -1   # no context
    assert n.value == 7 and not out.tobytes().strip(b"\0")
    fs = _abi.PsFrameSetF32()
    assert L.ps_match_l2_device(None, C.byref(fs), None, 1, None, None) == -1
    assert L.ps_vo_pairs_l2_device(None, None, None, None, C.byref(fs), None, 1, None) == -1
