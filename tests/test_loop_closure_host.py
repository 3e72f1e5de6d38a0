"""Host half of the batched loop-closure verification (no GPU): struct sizes against the library, the entry points' rejections
that need no device, and the sequential restatement of tests/loop_closure_ref.py against its brute-force formulation."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_closure_ref as lref  # noqa: E402

from putslam_amd import _lib  # noqa: E402
from putslam_amd._abi import (PS_SET_INVALID, PsFrameSet, PsLoopBatch, PsLoopResults, PsMapStore, PsPairResults, PsPoseSetOut,  # noqa: E402
                              PsPoseSetRequest, default_ransac_params, make_config)


def test_struct_sizes():
    L = _lib.load()
    sizes = _lib.struct_sizes()
    for name, cls in (("pose_set_request", PsPoseSetRequest), ("pose_set_out", PsPoseSetOut), ("loop_batch", PsLoopBatch),
                      ("loop_results", PsLoopResults)):
        assert getattr(L, "ps_abi_sizeof_" + name)() == C.sizeof(cls) == sizes[name], name
    assert C.sizeof(PsPoseSetRequest) == 24 and C.sizeof(PsPoseSetOut) == C.sizeof(PsFrameSet) + 24
    assert C.sizeof(PsLoopBatch) == C.sizeof(PsFrameSet) + 48 and C.sizeof(PsLoopResults) == C.sizeof(PsPairResults) + 40


def test_device_calls_reject_a_null_context():
    """Without a context there is nothing to run on and nowhere to leave an error text: PS_ERR_BAD_ARG, no GPU needed --
    whatever else the arguments hold (NULL blocks, S beyond PS_LOOP_MAX_SETS, L < 0)."""
    L = _lib.load()
    st, rq, out = PsMapStore(), PsPoseSetRequest(), PsPoseSetOut()
    assert L.ps_pose_sets_device(None, C.byref(st), C.byref(rq), C.byref(out)) == -1
    assert L.ps_pose_sets_device(None, None, None, None) == -1
    rq.S = 1025
    assert L.ps_pose_sets_device(None, C.byref(st), C.byref(rq), C.byref(out)) == -1
    prm, (cfg, _) = default_ransac_params(0, lc=True), make_config(0, 1157, seed=1)
    b, r = PsLoopBatch(), PsLoopResults()
    assert L.ps_loop_pairs_device(None, C.byref(prm), C.byref(cfg), None, C.byref(b), C.byref(r)) == -1
    assert L.ps_loop_pairs_device(None, None, None, None, None, None) == -1
    b.L = -1
    assert L.ps_loop_pairs_device(None, C.byref(prm), C.byref(cfg), None, C.byref(b), C.byref(r)) == -1


def test_sequential_restatement_equals_the_brute_force_formulation():
    rng = np.random.default_rng(733)
    for F, N, max_obs in ((1500, 40, 12), (700, 9, 6), (300, 3, 3), (0, 5, 4)):
        store, p3d = lref.make_scene(rng, F, N, max_obs=max_obs, extra_poses=2)
        poses = np.concatenate([rng.integers(0, N, 12), [N, N + 1, -1, N + 2, 0, 0]]).astype(np.int32)    # unobserved, bad, twice
        for cap in (F + 1, 20):
            a, b = lref.pose_sets(store, p3d, poses, cap), lref.pose_sets_fast(store, p3d, poses, cap)
            assert all(lref.sets_equal(x, y) for x, y in zip(a, b))
            counts = [x["setCount"] for x in a]
            assert counts[12] == counts[13] == 0 and counts[14] == counts[15] == PS_SET_INVALID
            assert lref.sets_equal(a[16], a[17])
            if F and cap == 20:
                assert min(c for c in counts if c != PS_SET_INVALID) < -20, counts                  # overflow: -(count)
            elif F:
                assert max(counts) > 20, counts
                w = max((x for x in a if x["rows"] is not None), key=lambda x: x["nkpts"])
                assert (np.diff(w["rows"]["featIdx"]) > 0).all()                       # ascending feature index
                assert (store["obs_pose"][w["rows"]["obsIdx"]] == store["obs_pose"][w["rows"]["obsIdx"][0]]).all()
    # a malformed store: two observations of one pose -> the first; an id outside the table -> nobody's; a bad range -> everything
    store, p3d = lref.make_scene(rng, 50, 8, max_obs=4)
    s2 = dict(store)
    s2["obs_pose"] = store["obs_pose"].copy()
    f = int(np.nonzero(np.diff(store["obs_start"]) >= 3)[0][0])
    o = int(store["obs_start"][f])
    s2["obs_pose"][o:o + 3] = [5, 5, 99]
    for fn in (lref.pose_sets, lref.pose_sets_fast):
        w = fn(s2, p3d, [5], 50)[0]
        k = int(np.nonzero(w["rows"]["featIdx"] == f)[0][0])
        assert w["rows"]["obsIdx"][k] == o
    for at, val in ((3, -1), (7, int(store["obs_start"][6]) - 1), (50, len(store["obs_pose"]) + 1)):
        s3 = dict(store)
        s3["obs_start"] = store["obs_start"].copy()
        s3["obs_start"][at] = val
        if lref._range_ok(s3):
            continue
        for fn in (lref.pose_sets, lref.pose_sets_fast):
            assert [x["setCount"] for x in fn(s3, p3d, [0, 1], 50)] == [PS_SET_INVALID] * 2


def test_gates_and_planted_loops_in_the_restatement(oracle):
    """The scene generator plants loops the restatement closes, and both gates and the -1.0 rule are reachable."""
    rng = np.random.default_rng(806)
    store, p3d = lref.make_scene(rng, 400, 6, max_obs=3, extra_poses=8)
    feats = lref.unpack(store, p3d)
    lref.plant_loop(rng, feats, 6, 7, range(0, 120))            # a true loop
    lref.observe(rng, feats, 8, range(100, 160))                # unrelated sets: run, rejected
    lref.observe(rng, feats, 9, range(200, 236))
    lref.observe(rng, feats, 10, range(300, 335))               # 35 = minNumberOfFeaturesLC: gated (strict)
    lref.observe(rng, feats, 11, range(340, 349))               # 9: the 10-feature rule under min = 5
    store, p3d = lref.pack(store, feats)
    poses = np.array([6, 7, 8, 9, 10, 11], np.int32)
    sets = lref.pose_sets(store, p3d, poses, 400)
    assert [s["setCount"] for s in sets] == [120, 120, 60, 36, 35, 9]
    prm = default_ransac_params(0, lc=True)
    cfg, _ = make_config(0, 1157, seed=7)
    pairs = np.array([[0, 1], [2, 3], [0, 4], [3, 5], [1, 0], [7, 0]], np.int32)
    K = np.array([525, 0, 319.5, 0, 525, 239.5, 0, 0, 1], np.float32)
    w = lref.verify(oracle, sets, pairs, prm, cfg, K, 35, 0.4, 400)
    assert w["state"] == [lref.RUN, lref.RUN, lref.GATED_MIN, lref.GATED_MIN, lref.RUN, lref.INVALID_PAIR]
    assert w["closed"].tolist() == [1, 0, 0, 0, 1, 0] and w["ratio"][0] > 0.8 and w["ratio"][2] == 0.0
    assert w["numPaired"][0] > 90 and w["numPaired"][5] == PS_SET_INVALID
    assert (w["paired_feat"][0][:, 0] == w["paired_feat"][0][:, 1]).mean() > 0.95      # the planted features pair with themselves
    w5 = lref.verify(oracle, sets, pairs, prm, cfg, K, 5, 0.4, 400)
    assert w5["state"] == [lref.RUN, lref.RUN, lref.RUN, lref.GATED_10, lref.RUN, lref.INVALID_PAIR]       # (3, 5): 9 > 5, but 9 < 10
