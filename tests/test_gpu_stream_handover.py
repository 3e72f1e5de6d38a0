"""The hand-over of a library call onto torch's current stream (device_batch._on_torch_stream) keeps torch's ORDER, not only
the results: a torch op queued just before the call writes the inputs' final values, a torch copy queued just after it reads the
outputs, nothing synchronises the host in between, and the copy must hold what a fully synchronised run computes -- from torch's
default stream (handle 0: forked to and joined from the side stream) and from an explicit stream (handed over as it is).

Four entry points have tests of their own below; then every asynchronous entry point runs its case of tests/stream_order_cases.py
the same way, pairs of calls run across a ps_context_set_stream while the first stream is still busy, and the front-end chain
detect -> thin -> gather -> describe -> track -> select is queued without a host step."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_order_cases as S  # noqa: E402

from putslam_amd import synth  # noqa: E402
from putslam_amd._abi import EST_FIXED, EUCLIDEAN_ERROR, TUM_FR1_K, default_ransac_params, make_config  # noqa: E402

pytestmark = pytest.mark.gpu

CAP, NK = 64, [40, 64]


BALLAST_BYTES, BALLAST_FILLS = 1 << 30, 64


@pytest.fixture(scope="module")
def ballast():
    import torch
    return torch.empty(BALLAST_BYTES, dtype=torch.uint8, device="cuda:0")


def _busy(ballast, times=1):
    """times x BALLAST_FILLS fills of the ballast on torch's current stream and an event behind them: while event.query() is False
    the stream is still busy with them, so whatever was queued behind is pending.  Returns (event, event in front of the fills).

    Measured on the MI355X (every run prints both figures, _report): 64 fills of 1 GiB take 9.9 - 10.0 ms between the two events.
    Queuing on the host (perf_counter around the call) takes 0.02 - 0.11 ms for a single entry point -- the slowest is the case of
    ps_orb_pyramids_build_device, a build and a describe --, up to 0.29 ms for the two calls and two ps_context_set_stream of a
    switch pair, and 0.52 - 0.70 ms for the whole front-end chain, the slowest thing queued here.  The ballast is 14 times that,
    where 4 times is asked for as the margin for a busy host; the four fills of 256 MiB this file used before come to about
    0.16 ms at that rate (not measured), no more than two single calls and a quarter of the chain."""
    import torch
    first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    first.record()
    for _ in range(times * BALLAST_FILLS):
        ballast.fill_(1)
    last.record()
    return last, first


def _report(what, first, last, host_seconds):
    print("%s: queued in %.3f ms on the host, ballast %.3f ms" % (what, host_seconds * 1e3, first.elapsed_time(last)))


@pytest.fixture(params=["default", "side"])
def ordered(request, ctx, ballast):
    """ordered(inputs, finals, call, outputs, drains=False) -> clones of outputs(), taken on the stream under test behind call(),
    which runs behind the copies finals -> inputs; the stream is busy before them (_busy), so that they are still pending when
    call() is made -- and that is checked: the event behind the ballast, read on the host right after call() returns, must not
    have happened ("ballast too short": the run proved nothing).  drains=True, a wrapper that synchronises the host before it
    queues: the event must have happened, so a host synchronisation is where the table says and nowhere else."""
    import time
    import torch
    stream = torch.cuda.Stream() if request.param == "side" else torch.cuda.default_stream()

    def run(inputs, finals, call, outputs, drains=False):
        torch.cuda.synchronize()
        if drains and request.param == "default":
            # the wrapper's synchronisation drains the default stream and leaves the side stream the call runs on idle, so a
            # missing join would go unnoticed: that stream is kept busy by a ballast of its own, three times as long (the two
            # run side by side and share the memory's bandwidth)
            from putslam_amd.device_batch import _work_stream
            with torch.cuda.stream(_work_stream(torch.device("cuda:0"))):
                _busy(ballast, 3)
        with S.quiet_collector(), torch.cuda.stream(stream):     # (no handle of an earlier test is destroyed inside the timed call)
            busy, first = _busy(ballast)
            for t, f in zip(inputs, finals):
                t.copy_(f)
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            drained = busy.query()
            got = [t.clone() for t in outputs()]
        torch.cuda.synchronize()
        _report(request.node.name, first, busy, t1 - t0)
        if drains:
            assert drained, "the wrapper no longer synchronises the host before it queues: correct the table's `drains`"
        else:
            assert not drained, "ballast too short (or the wrapper synchronised the host): the stream was idle when the call was queued"
        return got

    run.stream = stream
    yield run
    ctx.set_stream(0)


def _stale_and_final(arrays):
    """For every host array: a device tensor of zeros (a valid, empty input) and one with the final values."""
    import torch
    finals = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    return [torch.zeros_like(f) for f in finals], finals


def _check(got, want):
    import torch
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), k


def _kept(kept, nkept):
    """(kept, nkept) of a filter with the rows beyond each frame's count, which are not written, cleared."""
    import torch
    cols = torch.arange(kept.shape[1], device=kept.device)[None, :]
    return [torch.where(cols < nkept[:, None], kept, torch.zeros_like(kept)), nkept]


def test_run_pairs(ctx, ordered):
    import torch
    from putslam_amd.device_batch import FrameSetDevice, PairBatchDevice, run_pairs
    seq = synth.make_sequence(2, CAP, config=3, index=5100)
    prm = default_ransac_params(EUCLIDEAN_ERROR)
    cfg, _ = make_config(EST_FIXED, 64, seed=11)
    results = lambda b: [b.matches, b.num_matches, b.mask, b.pose, b.stats]   # noqa: E731
    fs, ref = FrameSetDevice(seq["desc"], seq["pts"], NK), PairBatchDevice([[0, 1]], CAP)
    run_pairs(ctx, prm, cfg, TUM_FR1_K, fs, ref)
    torch.cuda.synchronize()
    assert 0 < ref.num_matches.item() <= 40
    late, out = FrameSetDevice(np.zeros_like(seq["desc"]), np.zeros_like(seq["pts"]), [0, 0]), PairBatchDevice([[0, 1]], CAP)
    got = ordered([late.desc, late.pts, late.nkpts], [fs.desc, fs.pts, fs.nkpts],
                  lambda: run_pairs(ctx, prm, cfg, TUM_FR1_K, late, out), lambda: results(out))
    _check(got, results(ref))


def test_dbscan_thin_device(ctx, ordered):
    import torch
    from putslam_amd.device_batch import dbscan_thin_device
    rng = np.random.default_rng(5200)
    centres = rng.uniform(40.0, 600.0, (2, 8, 2))
    xy = (centres[np.arange(2)[:, None], rng.integers(0, 8, (2, CAP))] + rng.normal(0.0, 3.0, (2, CAP, 2))).astype(np.float32)
    xy[:, ::5] = rng.uniform(0.0, 640.0, (2, len(range(0, CAP, 5)), 2))          # (and some keypoints on their own)
    octave = rng.integers(0, 4, (2, CAP)).astype(np.int32)
    stale, final = _stale_and_final([xy, np.array(NK, np.int32), octave])
    want = dbscan_thin_device(ctx, final[0], final[1], final[2])
    torch.cuda.synchronize()
    nk = want[1].cpu().numpy()
    assert (0 < nk).all() and (nk < NK).all()
    res = []
    got = ordered(stale, final, lambda: res.extend(dbscan_thin_device(ctx, *stale[:2], stale[2])), lambda: res)
    _check(_kept(*got), _kept(*want))


def test_exclude_device(ctx, ordered):
    import torch
    from putslam_amd import api
    from putslam_amd.device_batch import exclude_device
    rng = np.random.default_rng(5300)
    e3 = (rng.uniform(-1.0, 1.0, (2, CAP, 3)) + [0, 0, 3.0]).astype(np.float32)
    e2 = rng.uniform(0.0, 600.0, (2, CAP, 2)).astype(np.float32)
    c3, c2 = e3.copy(), e2.copy()                       # every candidate on an existing feature, but for every other one
    c3[:, ::2] += rng.uniform(0.5, 1.0, (2, CAP // 2, 3)).astype(np.float32)
    c2[:, ::2] += np.float32(50.0)
    counts = np.array(NK, np.int32)
    rule = api.rule_new_map_features(0.03, 2.0, 200)
    stale, final = _stale_and_final([c3, c2, counts, e3, e2, counts])
    want = exclude_device(ctx, rule, *final)
    torch.cuda.synchronize()
    nk = want[1].cpu().numpy()
    assert (0 < nk).all() and (nk < NK).all()
    res = []
    got = ordered(stale, final, lambda: res.extend(exclude_device(ctx, rule, *stale)), lambda: res)
    _check(_kept(*got), _kept(*want))


def test_run_match_xyz(ctx, ordered):
    import torch
    from putslam_amd.device_batch import FrameSetDevice, MapBatchDevice, run_match_xyz
    seq = synth.make_sequence(1, CAP, config=3, index=5400)
    rng = np.random.default_rng(5400)
    vpos = seq["pts"] + rng.normal(0.0, 0.01, seq["pts"].shape).astype(np.float32)       # the view: the frame's keypoints,
    vdesc = seq["desc"] ^ np.packbits(rng.random((1, CAP, 256)) < 0.03, axis=2)          # a centimetre off, 3 % of the bits
    level = np.zeros((1, CAP), np.int32)

    def batch(maps, frames):
        return MapBatchDevice(maps, level, frames, level, [[0, 0]], 4 * CAP)

    views, frames = FrameSetDevice(vdesc, vpos, [CAP]), FrameSetDevice(seq["desc"], seq["pts"], [CAP])
    ref = batch(views, frames)
    run_match_xyz(ctx, ref)
    torch.cuda.synchronize()
    assert ref.num_matches.item() > 0
    late = [FrameSetDevice(np.zeros_like(vdesc), np.zeros_like(vpos), [0]) for _ in range(2)]
    out = batch(*late)
    got = ordered([t for s in late for t in (s.desc, s.pts, s.nkpts)], [t for s in (views, frames) for t in (s.desc, s.pts, s.nkpts)],
                  lambda: run_match_xyz(ctx, out), lambda: [out.matches, out.num_matches])
    _check(got, [ref.matches, ref.num_matches])


# ---------------------------------------------------------------- every asynchronous entry point, from the table
def _want(ctx, name, k):
    """What case k of an entry point computes with everything synchronised before and after the call.  Made anew in front of every
    run under test, not kept: the call also leaves the context as the run under test must find it -- the scratch arena grown to
    the case's size and the RANSAC stop table that of the case's parameters, for a call that has to grow the one or rebuild the
    other drains its stream first, as it should, and would read here as a host synchronisation in the wrapper."""
    import torch
    case = S.TABLE[name].prep(k, ctx)
    for t, f in zip(case.inputs, case.finals):
        t.copy_(f)
    torch.cuda.synchronize()
    case.call(ctx)
    torch.cuda.synchronize()
    assert bool((case.counts() > 0).all()), (name, k, case.counts())          # the expected run did something
    want = case.norm([t.clone() for t in case.outputs()])
    torch.cuda.synchronize()
    ctx.set_stream(0)
    return want


def _differ(a, b):
    import torch
    return any(not torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(S.TABLE))
def test_entry_point_keeps_the_order_of_torchs_stream(ctx, ordered, name):
    import torch
    entry = S.TABLE[name]
    want = _want(ctx, name, 0)
    case = entry.prep(0, ctx)
    torch.cuda.synchronize()
    got = ordered(case.inputs, case.finals, lambda: case.call(ctx), case.outputs, entry.drains)
    _check(case.norm(got), want)


# ---------------------------------------------------------------- across a stream switch, the first stream busy
def _switch(ctx, ballast, first, second):
    """first() on stream A behind the ballast, ps_context_set_stream to stream B with no synchronisation, second(); A must still
    be busy when second() has been queued.  The contexts' calls are made directly (direct=True): no wrapper chooses a stream."""
    import time
    import torch
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with S.quiet_collector():
        with torch.cuda.stream(a):
            busy, start = _busy(ballast)
        t0 = time.perf_counter()
        ctx.set_stream(a.cuda_stream)
        first()
        ctx.set_stream(b.cuda_stream)
        second()
        t1 = time.perf_counter()
        drained = busy.query()
    torch.cuda.synchronize()
    ctx.set_stream(0)
    _report("switch", start, busy, t1 - t0)
    assert not drained, "ballast too short: stream A was idle at the switch"


def _filled(case):
    import torch
    for t, f in zip(case.inputs, case.finals):
        t.copy_(f)
    torch.cuda.synchronize()
    return case


def _outputs(case):
    return case.norm([t.clone() for t in case.outputs()])


SAME_CALL = ["ps_match_l2_device", "ps_vo_pairs_l2_device", "ps_match_xyz_l2_device", "ps_map_pairs_l2_device", "ps_map_views_l2_device",
             "ps_pose_sets_device", "ps_pose_sets_l2_device", "ps_loop_pairs_device", "ps_loop_pairs_l2_device", "ps_klt_select_device",
             "ps_detect_features_device"]


@pytest.mark.parametrize("name", SAME_CALL)
def test_same_call_on_two_streams_with_the_first_busy(ctx, ballast, name):
    """Inputs 0 on stream A, inputs 1 on stream B: both results are those of two separate synchronised calls.  The two
    ps_detect_features_device calls share ONE detector (its maps and ROI lists): the first call's outputs must not hold the second
    image's key points."""
    want = [_want(ctx, name, 0), _want(ctx, name, 1)]
    assert _differ(want[0], want[1])
    prep = S.TABLE[name].prep
    one = _filled(prep(0, ctx))
    two = _filled(prep(1, ctx, share=one) if name == "ps_detect_features_device" else prep(1, ctx))
    _switch(ctx, ballast, lambda: one.call(ctx, direct=True), lambda: two.call(ctx, direct=True))
    _check(_outputs(one), want[0])
    _check(_outputs(two), want[1])


@pytest.mark.parametrize("name", ["ps_klt_pyramids_build_device", "ps_orb_pyramids_build_device"])
def test_build_on_one_stream_then_its_reader_on_another(ctx, ballast, name):
    """Read after write on the slots of a pyramid set, which belong to the set and not to a stream."""
    want = _want(ctx, name, 0)
    case = _filled(S.TABLE[name].prep(0, ctx))
    _switch(ctx, ballast, lambda: case.build(ctx, direct=True), lambda: case.read(ctx, direct=True))
    _check(_outputs(case), want)


@pytest.mark.parametrize("name", ["ps_klt_track_device", "ps_describe_features_device"])
def test_rebuild_on_another_stream_while_a_reader_is_queued(ctx, ballast, name):
    """Write after read: a track / describe of the slots' content queued on stream A, the same slots built again from other images
    on stream B.  The reader's result is the old content's; the same reader afterwards sees the new content."""
    import torch
    want = _want(ctx, name, 0)
    case = _filled(S.TABLE[name].prep(0, ctx))
    _switch(ctx, ballast, lambda: case.call(ctx, direct=True), lambda: case.rebuild(ctx, direct=True))
    _check(_outputs(case), want)
    case.call(ctx)
    torch.cuda.synchronize()
    ctx.set_stream(0)
    assert _differ(_outputs(case), want)


# ---------------------------------------------------------------- the front-end chain, queued without a host step
@pytest.fixture(scope="module")
def chain(ctx):
    c = S.ChainDevice(ctx)
    yield c
    c.close()


@pytest.fixture(scope="module")
def chain_stepwise(ctx, chain):
    """The chain with torch.cuda.synchronize() after every step, on the real images."""
    import torch
    images = torch.from_numpy(np.stack(S.chain_images())).to("cuda:0")
    torch.cuda.synchronize()
    out = chain.run(images, torch.cuda.synchronize)
    torch.cuda.synchronize()
    ctx.set_stream(0)
    return {k: t.cpu().numpy() for k, t in out.items()}


def test_chain_stepwise_equals_the_restatements_chained(chain_stepwise):
    g, ref, want = chain_stepwise, S.chain_reference(), S.CHAIN_COUNTS
    assert g["counts"].tolist() == want["detected"] and g["nkept"].tolist() == want["thinned"] and g["dnum"].tolist() == want["described"]
    for f, r in enumerate(ref["frames"]):
        n, m, d = len(r["xy"]), len(r["keep"]), len(r["kept"])
        assert g["xy"][f, :n].tobytes() == r["xy"].tobytes() and g["response"][f, :n].tobytes() == r["response"].tobytes(), f
        assert g["kept"][f, :m].tolist() == r["keep"].tolist() and g["kxy"][f, :m].tobytes() == r["kxy"].tobytes(), f
        assert g["dkept"][f, :d].tolist() == r["kept"].tolist() and g["desc"][f, :d].tobytes() == r["desc"].tobytes(), f
    m = want["thinned"][0]
    assert g["next"][0, :m].tobytes() == np.ascontiguousarray(ref["next"], np.float32).tobytes()
    assert g["status"][0, :m].tolist() == ref["status"].tolist() and int(g["status"].sum()) == want["tracked"]
    assert g["err"][0, :m].tobytes() == np.ascontiguousarray(ref["err"], np.float32).tobytes()
    s = want["selected"]
    assert int(g["num"][0]) == s and g["sidx"][0, :s].tolist() == ref["selected"].tolist()
    assert g["matches"][0, :s, :3].tolist() == ref["matches"].tolist()
    assert g["spts"][0, :s].tobytes() == np.ascontiguousarray(ref["next"], np.float32)[ref["selected"]].tobytes()


@pytest.mark.parametrize("where", ["default", "side"])
def test_chain_queued_without_a_host_step(ctx, ballast, chain, chain_stepwise, where):
    """The images arrive by a copy queued behind the ballast (stale: zero images, nothing detected); every link is queued while
    the stream is still busy with the ballast, a torch gather stands between two library calls, and the clones equal the stepwise
    run's, byte for byte."""
    import time
    import torch
    stream = torch.cuda.Stream() if where == "side" else torch.cuda.default_stream()
    final = torch.from_numpy(np.stack(S.chain_images())).to("cuda:0")
    images = torch.zeros_like(final)
    torch.cuda.synchronize()
    with S.quiet_collector(), torch.cuda.stream(stream):
        busy, start = _busy(ballast)
        images.copy_(final)
        t0 = time.perf_counter()
        out = chain.run(images)
        t1 = time.perf_counter()
        drained = busy.query()
    torch.cuda.synchronize()
    ctx.set_stream(0)
    _report("chain/" + where, start, busy, t1 - t0)
    assert not drained, "ballast too short: the stream was idle before the chain was queued"
    got = {k: t.cpu().numpy() for k, t in out.items()}
    assert got["counts"].tolist() == S.CHAIN_COUNTS["detected"] and int(got["num"][0]) == S.CHAIN_COUNTS["selected"]
    for k, w in chain_stepwise.items():
        assert got[k].tobytes() == w.tobytes(), k
