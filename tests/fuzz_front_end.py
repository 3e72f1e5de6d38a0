#!/usr/bin/env python3
"""Randomised soak of the image front end and of the tracking step's merge: KLT, FAST, ORB detection, ORB description and
ps_track_close_pairs against their CPU restatements (tests/klt_ref.py, fast_ref.py, orb_detect_ref.py, orb_ref.py,
track_close_ref.py) over drawn shapes, windows, grids, level counts, thresholds, strides and counts -- byte for byte, float words
as uint32, every output block sentinel-filled and checked beyond every count.  No tolerance anywhere.

Every family has draw_<family>(rng) -- a plain dict of scalars, lists and seeds, drawn without the GPU, from which <family>_inputs
rebuilds the arrays -- and run_<family>(iters, seed), which returns the number of draws in which device and restatement differ.  A
draw that differs is printed whole: <family>_inputs(draw) and compare_<family>(ctx, draw) replay it.  A draw that breaks a premise
of its restatement is drawn again before anything is launched; the dict says how often (`redraws`).

tests/test_gpu_fuzz_front_end_slice.py collects the slices SLICE_SEEDS x SLICE_DRAWS under `-m gpu`;
tests/test_fuzz_front_end_host.py shows on the restatements alone what those very draws reach.  Longer soaks by hand, one
process, stopping at the first HIP error:

    python tests/fuzz_front_end.py --family klt --iters 2000 --seed 1
    python tests/fuzz_front_end.py --family all --iters 500
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import fast_ref as F  # noqa: E402
import frame_assembly_ref as A  # noqa: E402
import klt_ref as K  # noqa: E402
import orb_detect_ref as D  # noqa: E402
import orb_ref as O  # noqa: E402
import track_close_ref as C  # noqa: E402
from image_frontend_util import u32, upload_images  # noqa: E402

f32 = np.float32
SLICE_SEEDS = (11, 2026)
SLICE_DRAWS = dict(klt=24, fast=40, orb_detect=40, orb_describe=40, merge=40)
FAMILIES = tuple(SLICE_DRAWS)

SENT_F = np.uint32(0x7FA55A5A)   # a NaN no computation produces
SENT_I = np.int32(-0x5A5A5A5B)
SENT_B = np.uint8(0xA5)
TILE = C.MERGE_TILE              # ps_track_merge_rows passes candidates, and stages what it sweeps them against, 256 at a time


def pick(rng, values, weights=None):
    values = list(values)
    p = None if weights is None else np.asarray(weights, np.float64) / float(np.sum(weights))
    v = values[int(rng.choice(len(values), p=p))]
    return v.item() if isinstance(v, np.generic) else v


def slice_draws(family, seed, n=None):
    """The draws run_<family>(n, seed) makes, in order (default: the GPU slice's)."""
    rng = np.random.default_rng(seed)
    draw = globals()["draw_" + family]
    return [draw(rng) for _ in range(SLICE_DRAWS[family] if n is None else n)]


def sentinel(shape, dtype):
    import torch
    if np.dtype(dtype) == np.uint8:
        a = np.full(shape, SENT_B, np.uint8)
    elif np.dtype(dtype) == np.int32:
        a = np.full(shape, SENT_I, np.int32)
    else:
        a = np.full(shape, SENT_F, np.uint32).view(np.float32)
    return torch.from_numpy(a).to("cuda:0")


def words_equal(got, want):
    return u32(got).tolist() == u32(want).tolist()


class Why(list):
    """the differences of one draw: note(condition, what...) records what failed and hands the condition back"""

    def note(self, cond, *what):
        if not cond and len(self) < 16:
            self.append(what)
        return bool(cond)


_MEMO = {}


def _memo(family, cfg, compute):
    """the reference of the draw made last, kept from the premise check in draw_<family> for the comparison that follows"""
    key = repr({k: v for k, v in cfg.items() if k != "redraws"})
    if _MEMO.get(family, (None, None))[0] != key:
        _MEMO[family] = (key, compute())
    return _MEMO[family][1]


def _soak(family, iters, seed, ctx, verbose, compare):
    """The loop every run_<family> is: draw, compare, count.  An exception -- a HIP error is one -- ends the run."""
    rng = np.random.default_rng(seed)
    draw = globals()["draw_" + family]
    t0, bad = time.time(), 0
    for it in range(iters):
        cfg = draw(rng)
        why = compare(ctx, cfg)
        if why:
            bad += 1
            print("MISMATCH", family, dict(it=it, seed=seed), "draw:", cfg, "differences:", list(why), flush=True)
        if verbose and (it + 1) % 20 == 0:
            print(f"{family}: {it + 1} draws, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
    return bad


def _context(ctx):
    if ctx is not None:
        return ctx, False
    from putslam_amd import api
    return api.Context(0), True


# ================================================================================================ klt
# ps_klt_track spreads a window row-major over a wave: qstep = 64 / (W cn), rstep = 64 % (W cn).  The three classes of W cn:
KLT_CLASSES = {
    "divides": [(w, 1) for w in (4, 8, 16)],                                                        # rstep 0
    "below": [(w, 1) for w in range(3, 32) if w not in (4, 8, 16)] + [(w, 3) for w in range(3, 22)],   # both steps at work
    "above": [(w, 3) for w in range(22, 32)],                                                       # qstep 0: a row is longer than a wave
}
KLT_COUNTS = (0, 1, 40, 63, 64, 65)


def klt_class(win, cn):
    return "divides" if 64 % (win * cn) == 0 else ("below" if win * cn < 64 else "above")


def draw_klt(rng):
    """The class of W cn first, then the window in it (W cn = 63 and 66, the two sides of the wave width, weighted up); rows and
    cols independent in win + 1 .. 140; P = 1 .. 3 pairs (slot 0 -> slot p + 1, each with its own shift of up to +-4 px) with ragged
    counts.  maxLevels, maxCount, eps, the eigenvalue threshold and the counts are weighted towards the values that let a walk
    run (few levels, many steps, a small eps, a low threshold, many points), so that a slice takes every exit and builds some
    pyramids in full; every value of the space is drawn."""
    cls = pick(rng, ("divides", "below", "above"))
    x = rng.random()
    if cls == "below" and x < 0.35:
        win, cn = 21, 3
    elif cls == "above" and x < 0.4:
        win, cn = 22, 3
    else:
        win, cn = pick(rng, KLT_CLASSES[cls])
    P = int(rng.integers(1, 4))
    return dict(cls=cls, win=win, cn=cn, rows=int(rng.integers(win + 1, 141)), cols=int(rng.integers(win + 1, 141)),
                max_levels=pick(rng, range(8), (2, 3, 3, 2, 1, 1, 1, 1)),
                flags=pick(rng, (0, K.USE_INITIAL_FLOW, K.GET_MIN_EIGENVALS, K.USE_INITIAL_FLOW | K.GET_MIN_EIGENVALS)),
                max_count=pick(rng, (0, 1, 2, 5, 30, 150), (1, 1, 1, 2, 4, 3)), eps=pick(rng, (0.0, 0.01, 0.3, 20.0), (3, 3, 1, 1)),
                min_eig=pick(rng, (1e-4, 0.05, 5.0), (4, 2, 1)),
                shifts=[(round(float(rng.uniform(-4, 4)), 2), round(float(rng.uniform(-4, 4)), 2)) for _ in range(P)],
                padded=bool(rng.integers(0, 2)), counts=[pick(rng, KLT_COUNTS, (1, 1, 2, 2, 2, 2)) for _ in range(P)],
                err_threshold=pick(rng, (0.5, 3.0, 1e9)), min_dist=pick(rng, (0.0, 1.5, 6.0)),
                tex_seed=int(rng.integers(0, 1 << 30)), pts_seed=int(rng.integers(0, 1 << 30)), redraws=0)


def klt_inputs(cfg):
    """(images: slot 0 and one shifted copy per pair; points per pair; the initial flow per pair or None)"""
    rows, cols, cn, win = cfg["rows"], cfg["cols"], cfg["cn"], cfg["win"]
    imgs = [K.smooth_texture(rows, cols, cn, seed=cfg["tex_seed"])]
    imgs += [K.smooth_texture(rows, cols, cn, seed=cfg["tex_seed"], shift=(-sx, -sy)) for sx, sy in cfg["shifts"]]
    pts, init = [], []
    for p, c in enumerate(cfg["counts"]):
        seed = cfg["pts_seed"] + p
        d = K.directed_points(win, rows, cols)
        q = np.concatenate([K.random_points(rows, cols, c - len(d), seed), d]) if c >= len(d) else K.random_points(rows, cols, c, seed)
        pts.append(q.astype(f32).reshape(-1, 2))
        if cfg["flags"] & K.USE_INITIAL_FLOW:
            flow = (q + np.random.default_rng(seed + 7919).uniform(-3, 3, q.shape)).astype(f32).reshape(-1, 2)
            if c >= 2:
                flow[1] = (np.nan, 4.0)
            init.append(flow)
    return imgs, pts, (init if cfg["flags"] & K.USE_INITIAL_FLOW else None)


def klt_reference(cfg, inputs=None, exits=None):
    """Per pair (nextPts, status, err, keptIdx, matches) of klt_ref.track and klt_ref.select_pairwise on its result."""
    imgs, pts, init = inputs or klt_inputs(cfg)
    out = []
    for p in range(len(cfg["counts"])):
        nxt, st, er = K.track(imgs[0], imgs[p + 1], pts[p], cfg["win"], cfg["max_levels"], cfg["max_count"], cfg["eps"], cfg["flags"],
                              cfg["min_eig"], next_pts=None if init is None else init[p], exits=exits)
        kept, matches = K.select_pairwise(nxt, st, er, cfg["err_threshold"], cfg["min_dist"])
        out.append((nxt, st, er, kept, matches))
    return out


def compare_klt(ctx, cfg):
    import torch
    from putslam_amd import device_batch
    from putslam_amd._abi import klt_params
    why = Why()
    inputs = imgs, pts, init = klt_inputs(cfg)
    want = klt_reference(cfg, inputs)
    rows, cols, cn, win = cfg["rows"], cfg["cols"], cfg["cn"], cfg["win"]
    params = klt_params(win, cfg["max_levels"], cfg["max_count"], cfg["eps"], cfg["flags"], cfg["min_eig"])
    pyr = device_batch.KltPyramids(ctx, rows, cols, cn, len(imgs), win, cfg["max_levels"])
    try:
        pyr.build(upload_images(imgs, cfg["padded"]))
        L = K.level_count(rows, cols, win, cfg["max_levels"])
        if why.note(pyr.num_levels == L + 1, "levels", pyr.num_levels, L + 1):
            for slot, img in enumerate(imgs):
                for l, lv in enumerate(K.build_pyramid(img, win, cfg["max_levels"])):
                    gi, gd, dims = pyr.level(slot, l)
                    why.note(dims == lv.shape[:2] and np.array_equal(gi, K.pad_image(lv, win)), "level image", slot, l)
                    why.note(np.array_equal(gd, K.pad_deriv(K.scharr(lv), win)), "level derivative", slot, l)
        P, cap = len(pts), max(1, max(cfg["counts"]))
        prev = np.zeros((P, cap, 2), f32)
        nxt = np.full((P, cap, 2), SENT_F, np.uint32).view(f32)
        for p in range(P):
            prev[p, :len(pts[p])] = pts[p]
            if init is not None:
                nxt[p, :len(pts[p])] = init[p]
        dev = torch.device("cuda:0")
        counts = torch.tensor(cfg["counts"], dtype=torch.int32, device=dev)
        pairs = torch.tensor([[0, p + 1] for p in range(P)], dtype=torch.int32, device=dev)
        nxt, st, er = torch.from_numpy(nxt).to(dev), sentinel((P, cap), np.uint8), sentinel((P, cap), np.float32)
        device_batch.track_klt_pairs(ctx, pyr, pairs, torch.from_numpy(prev).to(dev), counts, params, nxt, st, er)
        m, num, kp, ki = device_batch.select_tracked(ctx, nxt, st, er, counts, cfg["err_threshold"], cfg["min_dist"])
        torch.cuda.synchronize()
        nxt, st, er, m, num, kp, ki = (t.cpu().numpy() for t in (nxt, st, er, m, num, kp, ki))
    finally:
        pyr.close()
    for p, (wn, ws, we, kept, matches) in enumerate(want):
        n = cfg["counts"][p]
        bad = [i for i in range(n) if not words_equal(nxt[p, i], wn[i]) or st[p, i] != ws[i] or u32(er[p, i:i + 1])[0] != u32(we[i:i + 1])[0]]
        why.note(not bad, "track", p, bad[:6],
                 [(nxt[p, i].tolist(), wn[i].tolist(), int(st[p, i]), int(ws[i]), float(er[p, i]), float(we[i])) for i in bad[:2]])
        why.note((u32(nxt[p, n:]) == SENT_F).all() and (st[p, n:] == SENT_B).all() and (u32(er[p, n:]) == SENT_F).all(), "track wrote beyond its count", p)
        k = len(kept)
        if why.note(int(num[p]) == k, "selection count", p, int(num[p]), k):
            why.note(np.array_equal(ki[p, :k], kept), "selection keptIdx", p)
            why.note(np.array_equal(m[p, :k, :3], matches) and not m[p, :k, 3].any(), "selection matches", p)
            why.note(words_equal(kp[p, :k], wn[kept]), "selection keptPts", p)
    return why


def run_klt(iters, seed, ctx=None, verbose=True):
    """ps_klt_pyramids_build_device, ps_klt_track_device and ps_klt_select_device against klt_ref: every stored level, nextPts /
    status / err per pair, the selection on the result."""
    ctx, own = _context(ctx)
    try:
        return _soak("klt", iters, seed, ctx, verbose, compare_klt)
    finally:
        if own:
            ctx.close()


# ================================================================================================ fast
GRID_SIDE_MAX = 7
MAX_FEATURES = (0, 1, 20, 50, 500)


def grid_limit(side):
    return max(1, min(GRID_SIDE_MAX, side // 10))


def draw_fast(rng):
    """rows and cols 7 .. 140 (tiles of 32 with a 3-pixel ring: every residue), a grid whose ROI origins fall inside tiles, 1 .. 4
    frames of one shape, each a scene of fast_ref.SCENES."""
    rows, cols = int(rng.integers(7, 141)), int(rng.integers(7, 141))
    return dict(rows=rows, cols=cols, cn=pick(rng, (1, 3)), scenes=[pick(rng, tuple(F.SCENES)) for _ in range(int(rng.integers(1, 5)))],
                threshold=pick(rng, (-5, 0, 5, 10, 20, 40, 255, 300), (1, 1, 2, 5, 5, 2, 1, 1)), nms=bool(rng.random() < 0.7),
                grid_rows=int(rng.integers(1, grid_limit(rows) + 1)), grid_cols=int(rng.integers(1, grid_limit(cols) + 1)),
                max_features=pick(rng, MAX_FEATURES), padded=bool(rng.integers(0, 2)), redraws=0)


def fast_inputs(cfg):
    imgs = [F.SCENES[name](cfg["rows"], cfg["cols"]) for name in cfg["scenes"]]
    return imgs if cfg["cn"] == 1 else [F.colour(g, 17 + i) for i, g in enumerate(imgs)]


def fast_reference(cfg, imgs=None, max_features=None):
    """Per frame ((grey, score, corner), (xy, response))"""
    imgs = imgs or fast_inputs(cfg)
    mx = cfg["max_features"] if max_features is None else max_features
    return [(F.maps_closed(img, cfg["threshold"], cfg["grid_rows"], cfg["grid_cols"]),
             F.detect_closed(img, cfg["threshold"], cfg["nms"], cfg["grid_rows"], cfg["grid_cols"], mx)) for img in imgs]


def compare_fast(ctx, cfg):
    import torch
    from putslam_amd import device_batch
    from putslam_amd._abi import detect_params
    why = Why()
    imgs = fast_inputs(cfg)
    want = fast_reference(cfg, imgs)
    n_frames, cap = len(imgs), max(1, cfg["max_features"])
    p = detect_params(cfg["threshold"], cfg["nms"], cfg["grid_rows"], cfg["grid_cols"], cfg["max_features"])
    det = device_batch.FastDetector(ctx, cfg["rows"], cfg["cols"], cfg["cn"], n_frames)
    try:
        xy, resp, cnt = sentinel((n_frames, cap, 2), np.float32), sentinel((n_frames, cap), np.float32), sentinel((n_frames,), np.int32)
        device_batch.detect_features_batch(ctx, det, upload_images(imgs, cfg["padded"]), p, cap, xy, resp, cnt)
        torch.cuda.synchronize()
        xy, resp, cnt = xy.cpu().numpy(), resp.cpu().numpy(), cnt.cpu().numpy()
        maps = [det.maps(f) for f in range(n_frames)]
    finally:
        det.close()
    for f, ((wg, ws, wc), (wxy, wr)) in enumerate(want):
        g, s, c = maps[f]
        why.note(np.array_equal(g, wg), "grey", f, np.argwhere(g != wg)[:4].tolist())
        why.note(np.array_equal(c, wc), "corner", f, np.argwhere(c != wc)[:4].tolist())
        why.note(np.array_equal(s, ws), "score", f, np.argwhere(s != ws)[:4].tolist())
        n = len(wr)
        if why.note(int(cnt[f]) == n, "count", f, int(cnt[f]), n):
            why.note(words_equal(xy[f, :n], wxy.reshape(-1, 2)), "xy", f)
            why.note(words_equal(resp[f, :n], wr), "response", f)
            why.note((u32(xy[f, n:]) == SENT_F).all() and (u32(resp[f, n:]) == SENT_F).all(), "wrote beyond its count", f)
    return why


def run_fast(iters, seed, ctx=None, verbose=True):
    """ps_detect_features_device against fast_ref: the grey / score / corner maps (maps_closed) and the lists (detect_closed)."""
    ctx, own = _context(ctx)
    try:
        return _soak("fast", iters, seed, ctx, verbose, compare_fast)
    finally:
        if own:
            ctx.close()


# ================================================================================================ orb_detect
ORB_SCENES = ("texture", "noise256", "noise4", "tiled")
DEBUG_LEVELS_MAX = 16       # the per-level planes and survivor lists are read back where ROIs x levels is at most this


def orb_detect_premise(cfg):
    """orb_detect_ref builds every level of every ROI's pyramid (`assert r >= 1 and c >= 1`); the library refuses a grid and a
    level count that leave an empty level."""
    h, w = cfg["rows"] // cfg["grid_rows"], cfg["cols"] // cfg["grid_cols"]
    return all(r >= 1 and c >= 1 for r, c, _ in O.level_geometry(h, w, cfg["scale_factor"], cfg["n_levels"]))


def draw_orb_detect(rng):
    """rows and cols 63 .. 200 (level 0 has an interior from 63 on), the grid weighted towards 1 x 1 -- an ROI keeps a key point
    only where it is more than 62 pixels a side --, the thresholds and maxima towards the values that let key points through."""
    redraws = 0
    while True:
        rows, cols = int(rng.integers(63, 201)), int(rng.integers(63, 201))

        def side(s):
            return 1 if rng.random() < 0.85 else int(rng.integers(1, grid_limit(s) + 1))

        cfg = dict(rows=rows, cols=cols, cn=pick(rng, (1, 3)), scene=pick(rng, ORB_SCENES), n_features=pick(rng, (0, 1, 2, 12, 24, 500), (1, 1, 2, 4, 4, 4)),
                   scale_factor=pick(rng, (1.2, 1.5, 2.0), (3, 2, 1)), n_levels=int(rng.integers(1, 9)), fast_threshold=pick(rng, (0, 20, 255), (2, 8, 1)),
                   grid_rows=side(rows), grid_cols=side(cols), max_features=pick(rng, MAX_FEATURES, (1, 1, 4, 4, 4)),
                   padded=bool(rng.integers(0, 2)), frames=int(rng.integers(1, 3)), redraws=redraws)
        if orb_detect_premise(cfg):
            return cfg
        redraws += 1


def orb_detect_params(cfg):
    return D.params(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["fast_threshold"], cfg["grid_rows"], cfg["grid_cols"],
                    cfg["max_features"])


def orb_detect_inputs(cfg):
    """frame 0 is the scene; a second frame is the scene turned by 180 degrees"""
    img = D.image(cfg["scene"], cfg["rows"], cfg["cols"], cfg["cn"])
    return [img, np.ascontiguousarray(img[::-1, ::-1])][:cfg["frames"]]


def orb_detect_reference(cfg, imgs=None):
    """Per frame detect_closed's (xy, response, angle, octave, the levels of every ROI)"""
    return [D.detect_closed(img, orb_detect_params(cfg), want_levels=True) for img in (imgs or orb_detect_inputs(cfg))]


def compare_orb_detect(ctx, cfg):
    import torch
    from putslam_amd import device_batch
    from putslam_amd import _abi
    why = Why()
    imgs = orb_detect_inputs(cfg)
    want = orb_detect_reference(cfg, imgs)
    n_frames, cap = len(imgs), max(1, cfg["max_features"])
    p = _abi.orb_detect_params(cfg["n_features"], cfg["scale_factor"], cfg["n_levels"], cfg["fast_threshold"], cfg["grid_rows"], cfg["grid_cols"],
                               cfg["max_features"])
    det = device_batch.OrbDetector(ctx, cfg["rows"], cfg["cols"], cfg["cn"], n_frames, p)
    try:
        blocks = (sentinel((n_frames, cap, 2), np.float32), sentinel((n_frames, cap), np.float32), sentinel((n_frames, cap), np.float32),
                  sentinel((n_frames, cap), np.int32), sentinel((n_frames,), np.int32))
        device_batch.detect_features_orb_batch(ctx, det, upload_images(imgs, cfg["padded"]), p, cap, *blocks)
        torch.cuda.synchronize()
        xy, resp, ang, octv, cnt = (b.cpu().numpy() for b in blocks)
        if det.num_rois * cfg["n_levels"] <= DEBUG_LEVELS_MAX:
            for f in range(n_frames):
                for q, levels in enumerate(want[f][4]):
                    for l, lv in enumerate(levels):
                        got = det.level(f, q, l)
                        why.note(np.array_equal(got["raw"], lv["raw"]), "raw level", f, q, l)
                        why.note(np.array_equal(got["score"], lv["score"]), "score", f, q, l)
                        why.note(got["yx"].tolist() == ((lv["y"].astype(np.int64) << 16) | lv["x"]).tolist(), "first cut", f, q, l)
                        why.note(words_equal(got["response"], lv["response"]), "harris", f, q, l)
                        why.note(words_equal(got["angle"], lv["angle"]), "angle", f, q, l)
                        why.note(got["kept"].tolist() == lv["kept"].astype(np.uint8).tolist(), "second cut", f, q, l)
    finally:
        det.close()
    for f, (wxy, wr, wa, wo, _) in enumerate(want):
        n = len(wr)
        if why.note(int(cnt[f]) == n, "count", f, int(cnt[f]), n):
            why.note(words_equal(xy[f, :n], wxy.reshape(-1, 2)), "xy", f)
            why.note(words_equal(resp[f, :n], wr), "response", f)
            why.note(words_equal(ang[f, :n], wa), "angle", f)
            why.note(octv[f, :n].tolist() == wo.tolist(), "octave", f)
            why.note((u32(xy[f, n:]) == SENT_F).all() and (u32(resp[f, n:]) == SENT_F).all() and (u32(ang[f, n:]) == SENT_F).all()
                     and (octv[f, n:] == SENT_I).all(), "wrote beyond its count", f)
    return why


def run_orb_detect(iters, seed, ctx=None, verbose=True):
    """ps_orb_detect_frames against orb_detect_ref.detect_closed: every output column, and the levels where they are few."""
    ctx, own = _context(ctx)
    try:
        return _soak("orb_detect", iters, seed, ctx, verbose, compare_orb_detect)
    finally:
        if own:
            ctx.close()


# ================================================================================================ orb_describe
DESCRIBE_COUNTS = (0, 1, 63, 64, 65, 257)
REACH_MAX = 32              # orb_ref.describe's condition: no sample further than this outside its level


def draw_orb_describe(rng):
    """rows and cols 9 .. 140, four draws in five above 62 (nothing is described in a smaller image: those draws hold the device to
    an empty answer); 1 .. 3 slots, 1 .. 4 frames each naming a slot, key points of every octave, the named edge cases with them
    from 63 on."""
    redraws = 0
    while True:
        def side():
            return int(rng.integers(63, 141)) if rng.random() < 0.8 else int(rng.integers(9, 63))

        slots = int(rng.integers(1, 4))
        frames = int(rng.integers(1, 5))
        cfg = dict(rows=side(), cols=side(), cn=pick(rng, (1, 3)), scale_factor=pick(rng, (1.2, 1.5)), n_levels=int(rng.integers(1, 9)),
                   custom_pattern=bool(rng.integers(0, 2)), slots=slots, frame_slots=[int(rng.integers(0, slots)) for _ in range(frames)],
                   counts=[pick(rng, DESCRIBE_COUNTS) for _ in range(frames)], padded=bool(rng.integers(0, 2)),
                   img_seed=int(rng.integers(0, 1 << 30)), kp_seed=int(rng.integers(0, 1 << 30)), redraws=redraws)
        if orb_describe_reference(cfg)[2]["reach"] <= REACH_MAX:
            return cfg
        redraws += 1


def orb_describe_inputs(cfg):
    """(images per slot, pattern or None, frames [(slot, xy, angle, octave)])"""
    rows, cols, nl = cfg["rows"], cfg["cols"], cfg["n_levels"]
    imgs = [O.texture(rows, cols, cfg["img_seed"] + s) for s in range(cfg["slots"])]
    if cfg["cn"] == 3:
        imgs = [F.colour(g, 5 + s) for s, g in enumerate(imgs)]
    def random_keypoints(n, seed):
        if rows > 2 * O.EDGE + 1 and cols > 2 * O.EDGE + 1:
            return O.random_keypoints(n, rows, cols, nl, seed)
        r = np.random.default_rng(seed)      # no interior: anywhere in the image, all of them dropped
        return (np.stack([r.uniform(0, cols, n), r.uniform(0, rows, n)], axis=1).astype(f32), r.uniform(0, 360, n).astype(f32),
                r.integers(0, nl, n).astype(np.int32))

    frames = []
    for f, (slot, c) in enumerate(zip(cfg["frame_slots"], cfg["counts"])):
        seed = cfg["kp_seed"] + f
        e = O.edge_keypoints(rows, cols, nl)
        if c >= len(e[0]):
            r = random_keypoints(c - len(e[0]), seed)
            xy, ang, octv = (np.concatenate([a, b]) for a, b in zip(r, e))
        else:
            xy, ang, octv = random_keypoints(c, seed)
        frames.append((slot, xy.astype(f32).reshape(-1, 2), ang.astype(f32), octv.astype(np.int32)))
    return imgs, (O.corner_pattern() if cfg["custom_pattern"] else None), frames


def orb_describe_reference(cfg, inputs=None):
    """(pyramids per slot, [(desc, keptIdx)] per frame, the counters of all frames together)"""
    def compute():
        imgs, pattern, frames = inputs or orb_describe_inputs(cfg)
        pyrs = [O.pyramid(img, cfg["scale_factor"], cfg["n_levels"]) for img in imgs]
        cnt = O.new_counters()
        return pyrs, [O.describe(pyrs[slot], xy, ang, octv, pattern, cnt) for slot, xy, ang, octv in frames], cnt
    return _memo("orb_describe", cfg, compute)


def compare_orb_describe(ctx, cfg):
    import torch
    from putslam_amd import device_batch
    from putslam_amd._abi import orb_params
    why = Why()
    inputs = imgs, pattern, frames = orb_describe_inputs(cfg)
    pyrs, want, _ = orb_describe_reference(cfg, inputs)
    n_frames, cap = len(frames), max(1, max(cfg["counts"]))
    pyr = device_batch.OrbPyramids(ctx, cfg["rows"], cfg["cols"], cfg["cn"], cfg["slots"], orb_params(cfg["scale_factor"], cfg["n_levels"]), pattern)
    try:
        pyr.build(upload_images(imgs, cfg["padded"]))
        xy, ang, octv = np.zeros((n_frames, cap, 2), f32), np.zeros((n_frames, cap), f32), np.zeros((n_frames, cap), np.int32)
        for f, (_, x, a, o) in enumerate(frames):
            xy[f, :len(o)], ang[f, :len(o)], octv[f, :len(o)] = x, a, o
        dev = torch.device("cuda:0")
        desc = torch.full((n_frames, cap, 32), int(SENT_B), dtype=torch.uint8, device=dev)
        kept, num = sentinel((n_frames, cap), np.int32), sentinel((n_frames,), np.int32)
        device_batch.describe_features_batch(ctx, pyr, torch.tensor(cfg["frame_slots"], dtype=torch.int32, device=dev), torch.from_numpy(xy).to(dev),
                                             torch.from_numpy(ang).to(dev), torch.from_numpy(octv).to(dev),
                                             torch.tensor(cfg["counts"], dtype=torch.int32, device=dev), desc, kept, num)
        torch.cuda.synchronize()
        desc, kept, num = desc.cpu().numpy(), kept.cpu().numpy(), num.cpu().numpy()
        for s in range(cfg["slots"]):
            for l in range(cfg["n_levels"]):
                raw, blr = pyr.planes(s, l)
                why.note(raw.shape == pyrs[s][l][0].shape and raw.tobytes() == pyrs[s][l][0].tobytes(), "raw level", s, l)
                why.note(blr.tobytes() == pyrs[s][l][1].tobytes(), "blurred level", s, l)
    finally:
        pyr.close()
    for f, (wd, wk) in enumerate(want):
        k = len(wk)
        if why.note(int(num[f]) == k, "numKept", f, int(num[f]), k):
            why.note(kept[f, :k].tolist() == wk.tolist(), "keptIdx", f)
            why.note(desc[f, :k].tobytes() == wd.tobytes(), "desc", f, np.nonzero((desc[f, :k] != wd).any(axis=1))[0][:6].tolist())
            why.note((desc[f, k:] == SENT_B).all() and (kept[f, k:] == SENT_I).all(), "wrote beyond its count", f)
    return why


def run_orb_describe(iters, seed, ctx=None, verbose=True):
    """ps_orb_pyramids_build_device and ps_describe_features_device against orb_ref: every plane, desc, keptIdx and numKept."""
    ctx, own = _context(ctx)
    try:
        return _soak("orb_describe", iters, seed, ctx, verbose, compare_orb_describe)
    finally:
        if own:
            ctx.close()


# ================================================================================================ merge
TRACKED_COUNTS = (0, 24, 255, 256, 257, 300, 513)
CANDIDATE_COUNTS = (0, 1, 256, 257, 512, 513, 600, 1100)
ROW_NAMES = tuple(n for n, _, _ in C.COLUMNS)


def merge_inputs(cfg):
    """[(tracked rows, candidate rows or None)] per pair"""
    out = []
    for p in range(len(cfg["tracked"])):
        t = C.random_rows(cfg["tracked"][p], cfg["row_seed"] + p)
        nc = cfg["candidates"][p]
        if nc < 0:
            out.append((t, None))
            continue
        c = C.near_and_far_candidates(t, nc, cfg["row_seed"] + 100 + p, cfg["min_dist"])
        if nc > TILE:
            r = np.random.default_rng(cfg["row_seed"] + 200 + p)
            dst = np.nonzero(r.random(nc - TILE) < cfg["copy_share"])[0] + TILE
            src = (r.random(len(dst)) * ((dst // TILE) * TILE)).astype(np.int64)      # from a tile before dst's
            C.move_copies(c, src, dst, (1.0, 0.0))
        out.append((t, c))
    return out


def merge_reference(cfg, inputs=None, pyramids=None):
    """track_close_ref.close per pair"""
    def compute():
        pyr = pyramids or merge_pyramids(cfg["cn"])
        return [C.close(t, c, pyr[slot], cfg["cap"], cfg["minimal"], cfg["min_dist"]) for (t, c), slot in zip(inputs or merge_inputs(cfg), cfg["slots"])]
    return _memo("merge", cfg, compute)


_PYRAMIDS = {}


def merge_pyramids(cn):
    if cn not in _PYRAMIDS:
        _PYRAMIDS[cn] = [O.pyramid(img, C.SCALE_FACTOR, C.N_LEVELS) for img in A.images(cn)[:2]]
    return _PYRAMIDS[cn]


def merge_premise(want):
    """The device follows the description's keptIdx; the reference's position-matching walk selects the same rows unless a dropped
    row lies within 0.0001 px of the next described one (tests/test_track_close_ref_host.py)."""
    return all(w["walk"].tolist() == w["kept"].tolist() for w in want)


def draw_merge(rng):
    """P = 1 .. 3 pairs of one call: tracked and candidate counts on both sides of the tile seams, minimalTrackedFeatures one above
    pair 0's count (due) or at most it (not due) -- the other pairs fall where their counts put them --, one pair in ten without a
    candidate frame, a share of the candidates beyond the first tile copied from an earlier tile and moved by one pixel."""
    redraws = 0
    while True:
        P = int(rng.integers(1, 4))
        tracked = [pick(rng, TRACKED_COUNTS) for _ in range(P)]
        cand = [-1 if rng.random() < 0.1 else pick(rng, CANDIDATE_COUNTS, (1, 1, 1, 1, 1, 1, 2, 3)) for _ in range(P)]
        due = bool(rng.random() < 0.8)
        cfg = dict(tracked=tracked, candidates=cand, due=due, minimal=tracked[0] + 1 if due else int(rng.integers(0, tracked[0] + 1)),
                   min_dist=pick(rng, (0.0, 3.0, 10.0), (1, 3, 2)), cn=pick(rng, (1, 3)), slots=[int(rng.integers(0, 2)) for _ in range(P)],
                   cap=max(1, max(tracked)) + pick(rng, (0, 7)), ccap=max(1, max(cand)) + pick(rng, (0, 5)),
                   copy_share=round(float(rng.uniform(0.1, 0.3)), 3), row_seed=int(rng.integers(0, 1 << 30)), redraws=redraws)
        if merge_premise(merge_reference(cfg)):
            return cfg
        redraws += 1


def merge_seams(tracked, cand, want, min_dist):
    """What one pair's merge went through, on the restatement: (accepted candidates before the last tile, the rejected candidates
    that lie near no tracked row and near no accepted candidate of their own tile -- rejected only because of a candidate
    accepted in an EARLIER tile --, those of them that only the second trip over the accepted candidates rejects)."""
    if cand is None or want["refill"] != 1:
        return 0, [], []
    s = C.merge_seams(tracked, cand, min_dist)
    return s["before_last"], s["earlier_only"], s["second_trip_only"]


def fill_ee(*tensors):
    import torch
    for t in tensors:
        t.view(torch.uint8).fill_(0xEE)


def is_ee(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xEE).all())


def same_words(got, want):
    """bytes equal; where the expected float is a NaN the device's is one too"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if want.dtype.kind == "f":
        nan = np.isnan(want)
        if not np.array_equal(np.isnan(got), nan):
            return False
        got, want = got[~nan], want[~nan]
    return got.tobytes() == want.tobytes()


def compare_merge(ctx, cfg, device_pyramids=None):
    import torch
    from putslam_amd import device_batch as db
    from putslam_amd._abi import track_close_params
    from track_vo_util import dev
    why = Why()
    inputs = merge_inputs(cfg)
    want = merge_reference(cfg, inputs)
    P, cap, ccap = len(inputs), cfg["cap"], cfg["ccap"]
    ocap = cap + ccap
    own_pyr = device_pyramids is None
    pyr = db.OrbPyramids(ctx, A.ROWS, A.COLS, cfg["cn"], 2) if own_pyr else device_pyramids[cfg["cn"]]
    tc = db.TrackClose(ctx, P, ocap)
    try:
        if own_pyr:
            pyr.build(upload_images(A.images(cfg["cn"])[:2], True))
        t, c, out = db.TrackedRows(P, cap, "cuda:0"), db.FrameRowsDevice(P, ccap, "cuda:0"), db.ClosedRows(P, ocap, "cuda:0")
        fill_ee(*[getattr(t, n) for n in ROW_NAMES])
        fill_ee(*[getattr(c, n) for n in ROW_NAMES])
        fill_ee(out.desc, out.src_idx, out.refill, out.rows.counts, *[getattr(out.rows, n) for n in ROW_NAMES])
        for p, (tr, cr) in enumerate(inputs):
            for n in ROW_NAMES:
                if len(tr["xy"]):
                    getattr(t, n)[p, :len(tr["xy"])] = dev(np.asarray(tr[n]))
                if cr is not None and len(cr["xy"]):
                    getattr(c, n)[p, :len(cr["xy"])] = dev(np.asarray(cr[n]))
        t.counts.copy_(dev(np.array(cfg["tracked"], np.int32)))
        c.nkpts.copy_(dev(np.array([max(k, 0) for k in cfg["candidates"]], np.int32)))
        frame = dev(np.array([p if k >= 0 else -1 for p, k in enumerate(cfg["candidates"])], np.int32))
        torch.cuda.synchronize()
        db.track_close_pairs(ctx, tc, pyr, dev(np.array(cfg["slots"], np.int32)), t, c, frame, track_close_params(cfg["minimal"], cfg["min_dist"]),
                             out=out)
        torch.cuda.synchronize()
        got = out.download()
    finally:
        tc.close()
        if own_pyr:
            pyr.close()
    for p, w in enumerate(want):
        k = len(w["xy"])
        if not why.note(int(got["rows"]["counts"][p]) == k and int(got["refill"][p]) == w["refill"], "count / refill", p,
                        int(got["rows"]["counts"][p]), k, int(got["refill"][p]), w["refill"]):
            continue
        why.note(same_words(got["desc"][p, :k], w["desc"]), "desc", p)
        why.note(same_words(got["src_idx"][p, :k], w["src_idx"]), "srcIdx", p,
                 np.nonzero(got["src_idx"][p, :k] != w["src_idx"])[0][:6].tolist())
        why.note(is_ee(got["desc"][p, k:]) and is_ee(got["src_idx"][p, k:]), "wrote beyond its count", p)
        for n, dt, _ in C.COLUMNS:
            why.note(same_words(got["rows"][n][p, :k], np.asarray(w[n], dt)), n, p)
            why.note(is_ee(got["rows"][n][p, k:]), n + " beyond its count", p)
    return why


def run_merge(iters, seed, ctx=None, verbose=True):
    """ps_track_close_pairs against track_close_ref.close: srcIdx, the closed rows, desc and refill (the merge and the levels are
    read through them)."""
    from putslam_amd import device_batch as db
    ctx, own = _context(ctx)
    pyrs = {}
    try:
        for cn in (1, 3):
            pyrs[cn] = db.OrbPyramids(ctx, A.ROWS, A.COLS, cn, 2)
            pyrs[cn].build(upload_images(A.images(cn)[:2], True))
        return _soak("merge", iters, seed, ctx, verbose, lambda c, cfg: compare_merge(c, cfg, pyrs))
    finally:
        for h in pyrs.values():
            h.close()
        if own:
            ctx.close()


# ================================================================================================ command line
def main():
    import faulthandler
    faulthandler.enable()
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--family", default="all", choices=FAMILIES + ("all",))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    from putslam_amd import api
    ctx = api.Context(0)
    bad = 0
    for family in (FAMILIES if a.family == "all" else (a.family,)):
        n = globals()["run_" + family](a.iters, a.seed, ctx=ctx)      # (an exception -- a HIP error -- ends everything here)
        print(f"fuzz done: {family}, {a.iters} draws, {n} mismatches", flush=True)
        bad += n
    ctx.close()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
