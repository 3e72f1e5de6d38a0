#!/usr/bin/env python3
"""Randomised soak of the per-feature back end: sub-pixel patch alignment (ps_patch_models, ps_patch_align), measurement
uncertainty (ps_feature_uncertainty, ps_measurement_edges) and frame assembly (ps_gather_keypoints, ps_assemble_frames) against
their CPU restatements (tests/patches_ref.py, uncertainty_ref.py, frame_assembly_ref.py on the oracle) over drawn patch sizes,
image shapes, paddings, cameras, depth scales, sensors, counts, masks and output subsets -- byte for byte, float words as integers,
NaNs canonical where the headers say so, every output block sentinel-filled and checked beyond every count.  No tolerance anywhere.

The conventions are tests/fuzz_front_end.py's: draw_<family>(rng) is a plain dict made without the GPU, <family>_inputs(draw)
rebuilds the arrays, compare_<family>(ctx, draw) replays the draw and returns its differences, run_<family>(iters, seed) counts
the draws that differ and prints each whole.  A draw that breaks a premise of its restatement is drawn again (`redraws`).

tests/test_gpu_fuzz_back_end_slice.py collects the slices SLICE_SEEDS x SLICE_DRAWS under `-m gpu`;
tests/test_fuzz_back_end_host.py shows on the restatements alone what those very draws reach, and that named mutants of the
restatements differ from them on those draws.  Longer soaks by hand, one process, stopping at the first HIP error:

    python tests/fuzz_back_end.py --family patches --iters 2000 --seed 1
    python tests/fuzz_back_end.py --family all --iters 500
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

import frame_assembly_ref as A  # noqa: E402
import patches_ref as R  # noqa: E402
import uncertainty_ref as U  # noqa: E402
from fuzz_front_end import SENT_B, SENT_F, SENT_I, Why, _context, pick, same_words  # noqa: E402

f32, f64 = np.float32, np.float64
SLICE_SEEDS = (11, 2026)
SLICE_DRAWS = dict(patches=40, uncertainty=24, edges=24, assemble=24)
FAMILIES = tuple(SLICE_DRAWS)

SENT_D = np.uint64(0x7FF5A5A5A5A5A5A5)      # a double NaN no computation produces
PAD16, PAD8 = 0xEEEE, 0xEE                  # what lies between the rows and the frames of a padded block
_FILL = {np.dtype(np.uint8): (SENT_B, np.uint8), np.dtype(np.int32): (SENT_I, np.int32), np.dtype(np.float32): (SENT_F, np.uint32),
         np.dtype(np.float64): (SENT_D, np.uint64)}


def slice_draws(family, seed, n=None):
    """The draws run_<family>(n, seed) makes, in order (default: the GPU slice's)."""
    rng = np.random.default_rng(seed)
    draw = globals()["draw_" + family]
    return [draw(rng) for _ in range(SLICE_DRAWS[family] if n is None else n)]


def filled_host(shape, dtype):
    fill, word = _FILL[np.dtype(dtype)]
    return np.full(shape, fill, word).view(dtype)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def filled(shape, dtype):
    return dev(filled_host(shape, dtype))


def untouched(a):
    a = np.ascontiguousarray(a)
    fill, word = _FILL[a.dtype]
    return bool((a.view(word) == fill).all())


def bits_equal(got, want):
    """the same shape, type and bytes"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def strided_block(frames, row_pad, frame_pad, fill):
    """frames: equal arrays (rows, cols[, cn]) of uint8 or uint16 -> the device view (F, rows, cols[, cn]) into a block whose rows lie
    row_pad elements and whose frames frame_pad elements further apart than their content; the padding holds `fill`"""
    import torch
    a = np.stack(frames)
    F, rows = a.shape[:2]
    inner = int(np.prod(a.shape[2:]))
    row, frame = inner + row_pad, rows * (inner + row_pad) + frame_pad
    flat = np.full(F * frame, fill, a.dtype)
    for f in range(F):
        flat[f * frame:f * frame + rows * row].reshape(rows, row)[:, :inner] = a[f].reshape(rows, inner)
    t = dev(flat.view(np.int16) if a.dtype == np.uint16 else flat)
    return torch.as_strided(t, a.shape, (frame, row) + ((a.shape[3], 1) if a.ndim == 4 else (1,)))


_MEMO = {}


def _memo(family, cfg, compute):
    """the reference of the draw made last, kept for the comparison (or the second question) that follows"""
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


def _run(family, iters, seed, ctx, verbose, compare):
    ctx, own = _context(ctx)
    try:
        return _soak(family, iters, seed, ctx, verbose, compare)
    finally:
        if own:
            ctx.close()


# ================================================================================================ patches
# ps_patch_align gives one wave to a point and as many waves to a work-group as 64 KiB of LDS hold; a wave covers E = patchSize^2
# elements 64 at a time.  The classes of a patch size: (waves of a work-group, E < 64)
PATCH_CLASSES = {(4, True): [3, 5, 7], (4, False): list(range(9, 24, 2)), (3, False): [25, 27], (2, False): [29, 31]}
PATCH_CLASS_WEIGHTS = {(4, True): 2, (4, False): 3, (3, False): 3, (2, False): 2}
PATCH_CAPS = (1, 2, 3, 4, 5, 7, 8, 9, 13, 64, 65)
PATCH_CAP_WEIGHTS = (1, 3, 2, 1, 1, 1, 1, 2, 1, 1, 1)      # (the remainders against 3 and against 4 about as often as each other)
PATCH_SHAPES = ("fused_model", "fused_null", "two_calls")
FLAT_MARGIN = 6              # the flat block is planted where the image is this much larger than it


def patch_wave_bytes(ps):
    """ps_patches_rule.h: the patch as E4 doubles and five float rows of E4, E4 = E rounded up to a multiple of four"""
    return ((ps * ps + 3) & ~3) * 28


def patch_block_waves(ps):
    """ps_patches_rule.h: as many waves as 64 KiB of LDS hold, four at most"""
    return min(4, 65536 // patch_wave_bytes(ps))


def patch_class(ps):
    return patch_block_waves(ps), ps * ps < 64


def points_reached(cap, n, waves, index_waves=None, past=False):
    """The points of one pair that a launch of ceil(cap / waves) work-groups of `waves` waves reaches, in ps_patches.h's words: i =
    (block % bpp) * waves + w, taken where `i >= n` does not turn it away.  index_waves and past state the two mutants
    tests/test_fuzz_back_end_host.py holds the draws against: the index built with another wave count, and `i > n`."""
    if n < 0 or n > cap:
        return []
    iw = waves if index_waves is None else index_waves
    bpp = (cap + waves - 1) // waves
    reached = [b * iw + w for b in range(bpp) for w in range(waves)]
    return sorted(i for i in reached if not ((i > n) if past else (i >= n)))


def draw_patches(rng):
    """The class of the patch size first, then the size in it; rows and cols independent in 2h + 1 .. 2h + 60 (below 2h + 3 no old
    position has its taps inside: every point has status 5); 1 or 3 channels, rows 0 .. 7 bytes and frames 0 .. 40 bytes apart, 1 ..
    3 frames (frame k is the texture read at a drawn shift); P = 1 .. 5 pairs whose slots are drawn one by one -- repeats, -1 and
    `frames` among them --; a capacity that leaves every remainder against 3 and 4 waves; counts around 0 and the capacity; in
    half the draws the starts of the points without a name lie up to h + 1 pixels off (a walk longer than h is status 4)."""
    classes = list(PATCH_CLASSES)
    cls = pick(rng, classes, [PATCH_CLASS_WEIGHTS[c] for c in classes])
    ps = pick(rng, PATCH_CLASSES[cls])
    h = R.half(ps)
    frames, P, cap = int(rng.integers(1, 4)), int(rng.integers(1, 6)), pick(rng, PATCH_CAPS, PATCH_CAP_WEIGHTS)

    def slot():
        return int(rng.integers(0, frames)) if rng.random() < 0.85 else pick(rng, (-1, frames))

    return dict(cls=list(cls), ps=ps, rows=2 * h + 1 + int(rng.integers(0, 60)), cols=2 * h + 1 + int(rng.integers(0, 60)), cn=pick(rng, (1, 3)),
                row_pad=int(rng.integers(0, 8)), frame_pad=int(rng.integers(0, 41)), frames=frames,
                shifts=[(0, 0)] + [(int(rng.integers(-2, 3)), int(rng.integers(-2, 3))) for _ in range(frames - 1)],
                pairs=[(slot(), slot()) for _ in range(P)], cap=cap,
                counts=[pick(rng, (-1, 0, 1, cap - 1, cap, cap + 1), (1, 1, 2, 3, 4, 1)) for _ in range(P)],
                max_iter=pick(rng, (0, 1, 3, 50), (1, 1, 2, 4)), min_inc=pick(rng, (0.0, 5e-7, 0.04, 1e9), (2, 3, 3, 2)),
                flat=bool(rng.integers(0, 2)), far=bool(rng.integers(0, 2)), shape=pick(rng, PATCH_SHAPES), tex_seed=int(rng.integers(0, 1 << 30)),
                pts_seed=int(rng.integers(0, 1 << 30)), redraws=0)


def patch_points(rng, n, rows, cols, h):
    """patches_ref.drawn_points; in an image of 2h + 1 rows or cols, which has no inside to draw from, positions anywhere in it"""
    if rows >= 2 * h + 2 and cols >= 2 * h + 2:
        return R.drawn_points(rng, n, rows, cols, h)
    old = np.stack([rng.uniform(0, cols, n), rng.uniform(0, rows, n)], 1)
    pts = np.concatenate([old, old + rng.uniform(-2, 2, (n, 2))], 1)
    pts[0] = (h + 1, h + 1, h, h)
    pts[1, :2] = (np.inf, h)
    pts[2, 2:] = (np.nan, h)
    return pts


def patches_inputs(cfg):
    """dict(images: the frames, grey: their grey values, old / new (P, cap, 2) float64 whose rows beyond a count hold the sentinel,
    n: the rows of each pair that are points)"""
    rows, cols, ps, cap = cfg["rows"], cfg["cols"], cfg["ps"], cfg["cap"]
    h = R.half(ps)
    imgs = [R.smooth_texture(rows, cols, cfg["tex_seed"], cfg["cn"], shift=s) for s in cfg["shifts"]]
    side = 2 * h + 3                                                   # the taps of the patch and of its gradient
    flat = cfg["flat"] and rows >= side + FLAT_MARGIN and cols >= side + FLAT_MARGIN
    if flat:
        imgs[0][:side, :side] = 77
    P = len(cfg["pairs"])
    old, new, ns = filled_host((P, cap, 2), f64), filled_host((P, cap, 2), f64), []
    for p, c in enumerate(cfg["counts"]):
        n = c if 0 <= c <= cap else 0
        rng = np.random.default_rng(cfg["pts_seed"] + p)
        pts = patch_points(rng, max(n, 13) + 8, rows, cols, h)            # (the named points, the flat one, and eight more at least)
        if cfg["far"]:                                                   # the starts of the others up to h + 1 pixels off
            pts[13:, 2:] = pts[13:, :2] + rng.uniform(-(h + 1), h + 1, pts[13:, 2:].shape)
        if flat:
            pts[12] = (h + 1.5, h + 1.25, h + 2.0, h + 1.5)            # inside frame 0's flat block: a NaN inverse Hessian
        pts = pts[rng.permutation(len(pts))][:n]                         # (so that a short list is not the first named points)
        old[p, :n], new[p, :n] = pts[:, :2], pts[:, 2:]
        ns.append(n)
    return dict(images=imgs, grey=[R.grey(i) for i in imgs], old=old, new=new, n=ns)


def patches_reference(cfg, inputs=None):
    """Per pair dict(n, status, iterations, new: the fused call; model: per point None or the (patch, gx, gy, inv) it writes -- nothing
    where either slot lies outside --; model_status, pass_model: what ps_patch_models says of the pair's old slot and writes;
    given_status, given_iterations, given_new: ps_patch_align on that model)"""
    def compute():
        inp = inputs or patches_inputs(cfg)
        g, ps, frames = inp["grey"], cfg["ps"], cfg["frames"]
        out = []
        for p, (s0, s1) in enumerate(cfg["pairs"]):
            n = inp["n"][p]
            w = dict(n=n, status=np.zeros(n, np.uint8), iterations=np.zeros(n, np.int32), new=inp["new"][p, :n].copy(), model=[None] * n,
                     pass_model=[None] * n, model_status=np.full(n, R.OLD_TAPS_OUTSIDE, np.uint8))
            ok0, ok1 = 0 <= s0 < frames, 0 <= s1 < frames
            for k in range(n):
                (ox, oy), (nx, ny) = inp["old"][p, k], inp["new"][p, k]
                if ok0 and ok1:
                    st, x, y, it, m = R.align(g[s0], g[s1], ox, oy, nx, ny, ps, cfg["max_iter"], cfg["min_inc"])
                    if it > 0:
                        w["new"][k] = (x, y)
                    w["status"][k], w["iterations"][k], w["model"][k], w["pass_model"][k] = st, it, m, m
                    w["model_status"][k] = R.OLD_TAPS_OUTSIDE if m is None else (R.NAN_HESSIAN if np.isnan(m[3][0, 0]) else R.CONVERGED)
                else:
                    w["status"][k] = R.OLD_TAPS_OUTSIDE            # a slot outside the set fails the pair's points
                    if ok0:                                          # (the model pass looks at the old slot alone)
                        st, *m = R.model(g[s0], ox, oy, ps)
                        w["model_status"][k], w["pass_model"][k] = st, (None if st == R.OLD_TAPS_OUTSIDE else tuple(m))
            # PS_PATCH_GIVEN_MODEL: the old slot is not looked at; a point whose model rows still hold the sentinel -- NaN -- has a
            # NaN inverse Hessian, which is status 2 before any step
            w["given_status"], w["given_iterations"], w["given_new"] = w["status"].copy(), w["iterations"].copy(), w["new"].copy()
            for k in range(n):
                if ok1 and w["pass_model"][k] is None:
                    w["given_status"][k], w["given_iterations"][k], w["given_new"][k] = R.NAN_HESSIAN, 0, inp["new"][p, k]
            out.append(w)
        return out
    return _memo("patches", cfg, compute)


def compare_patches(ctx, cfg):
    import torch
    from putslam_amd import device_batch as D
    from putslam_amd._abi import patch_params
    why = Why()
    inp = patches_inputs(cfg)
    want = patches_reference(cfg, inp)
    P, cap, ps = len(cfg["pairs"]), cfg["cap"], cfg["ps"]
    E = ps * ps
    params = patch_params(ps, cfg["max_iter"], cfg["min_inc"])
    imgs = strided_block(inp["images"], cfg["row_pad"], cfg["frame_pad"], PAD8)
    pairs, counts = dev(np.array(cfg["pairs"], np.int32).reshape(P, 2)), dev(np.array(cfg["counts"], np.int32))
    new_t, st, it = dev(inp["new"]), filled((P, cap), np.uint8), filled((P, cap), np.int32)
    model = mst = None
    if cfg["shape"] != "fused_null":
        model = D.PatchModels(P, cap, ps, torch.device("cuda:0"), want=())
        model.patch, model.gx, model.gy, model.inv = filled((P, cap, E), f64), filled((P, cap, E), f32), filled((P, cap, E), f32), filled((P, cap, 9), f32)
    torch.cuda.synchronize()
    if cfg["shape"] == "two_calls":
        mst = filled((P, cap), np.uint8)
        D.patch_models(ctx, imgs, dev(np.array([s0 for s0, _ in cfg["pairs"]], np.int32)), dev(inp["old"]), counts, params, model, mst)
        D.align_patches(ctx, imgs, pairs, None, new_t, counts, params, model, given=True, status=st, iterations=it)
    else:
        D.align_patches(ctx, imgs, pairs, dev(inp["old"]), new_t, counts, params, model, status=st, iterations=it)
    torch.cuda.synchronize()
    new, st, it = new_t.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()
    arrays = [t.cpu().numpy() for t in (model.patch, model.gx, model.gy, model.inv)] if model else []
    mst = mst.cpu().numpy() if mst is not None else None
    pre = "given_" if cfg["shape"] == "two_calls" else ""
    for p, w in enumerate(want):
        n = w["n"]
        why.note(bits_equal(new[p, n:], inp["new"][p, n:]) and untouched(st[p, n:]) and untouched(it[p, n:]), "wrote beyond its count", p)
        why.note(all(untouched(a[p, n:]) for a in arrays), "model written beyond its count", p)
        bad = [k for k in range(n) if (int(st[p, k]), int(it[p, k])) != (int(w[pre + "status"][k]), int(w[pre + "iterations"][k]))
               or not bits_equal(new[p, k], w[pre + "new"][k])]
        why.note(not bad, "status / iterations / position", p, bad[:6],
                 [(int(st[p, k]), int(w[pre + "status"][k]), int(it[p, k]), int(w[pre + "iterations"][k]), new[p, k].tolist(), w[pre + "new"][k].tolist())
                  for k in bad[:2]])
        if mst is not None:
            why.note(mst[p, :n].tolist() == w["model_status"].tolist() and untouched(mst[p, n:]), "model status", p)
        if model:
            for k in range(n):
                m = w["pass_model" if cfg["shape"] == "two_calls" else "model"][k]
                if m is None:
                    why.note(all(untouched(a[p, k]) for a in arrays), "a model where there is none", p, k)
                else:
                    why.note(all(bits_equal(a[p, k], b.reshape(-1)) for a, b in zip(arrays, m)), "model", p, k)
    return why


def run_patches(iters, seed, ctx=None, verbose=True):
    """ps_patch_align fused (the model written or not) and ps_patch_models followed by ps_patch_align on the given model, against
    patches_ref.align and patches_ref.model: positions, status, iterations and every model array."""
    return _run("patches", iters, seed, ctx, verbose, compare_patches)


# ================================================================================================ the scene of uncertainty and edges
HOLES = (0.0, 0.3, 0.6, 0.85, 1.0)
DEPTH_SCALES = (5000.0, 1000.0, 1.0, 3.7)          # (3.7 is no float: a division in float would show)
SPECIALS = (np.nan, np.inf, -np.inf, 2147483520.0, -2147483648.0, 3e9)
MEMBERS = ("normal", "gradient", "info")
SENSOR_SCALED = dict(scaleUncertaintyNormal=3.0, scaleUncertaintyGradient=0.25)
TIE_WORDS = {(1, 1): (2, 2), (-1, 1): (0, 2), (-1, -1): (0, 0), (1, -1): (2, 0)}      # (sgn gradx, sgn grady): the patch word to set


def draw_scene(rng):
    """What ps_feature_uncertainty and ps_measurement_edges look at: 1 .. 3 depth frames of 3 .. 24 rows and 3 .. 28 cols (one draw in
    eight has 3 rows or 3 cols: no pixel passes the gradient's border guard) with drawn holes, an image set of as many frames or
    fewer, each noise, a constant or zeros with a byte planted for each diagonal tie; both sets padded; a drawn camera, depth
    scale, sensor and model."""
    rows, cols = int(rng.integers(3, 25)), int(rng.integers(3, 29))
    if rng.random() < 0.125:
        rows, cols = (3, cols) if rng.random() < 0.5 else (rows, 3)
    D = int(rng.integers(1, 4))
    I = D if rng.random() < 0.6 else int(rng.integers(1, D + 1))
    kind = pick(rng, ("default", "scaled", "drawn"))
    sensor = {} if kind == "default" else dict(SENSOR_SCALED)
    if kind == "drawn":
        lo_hi = dict(fu=(100, 700), fv=(100, 700), cu=(0, 600), cv=(0, 600), varU=(0.1, 2), varV=(0.1, 2), c3=(1e-6, 1e-2), c2=(1e-6, 1e-2),
                     c1=(1e-6, 1e-2), c0=(1e-6, 1e-2), scaleUncertaintyNormal=(0.1, 5), scaleUncertaintyGradient=(0.1, 5))
        sensor = {k: float(rng.uniform(*lo_hi[k])) for k in U.SENSOR_FIELDS}
    flt = lambda v: float(f32(v))   # noqa: E731
    return dict(rows=rows, cols=cols, depth_frames=D, image_frames=I,
                K=[flt(rng.uniform(5, 600)), 0.0, flt(rng.uniform(0, cols)), 0.0, flt(rng.uniform(5, 600)), flt(rng.uniform(0, rows)), 0.0, 0.0, 1.0],
                scale=pick(rng, DEPTH_SCALES), holes=[pick(rng, HOLES) for _ in range(D)], depth_range=pick(rng, ("near", "full")),
                colour=[pick(rng, ("noise", "constant", "ties")) for _ in range(I)],
                depth_pad=(int(rng.integers(0, 6)), int(rng.integers(0, 41))), image_pad=(int(rng.integers(0, 8)), int(rng.integers(0, 41))),
                model=int(rng.integers(-1, 3)), sensor=sensor, scene_seed=int(rng.integers(0, 1 << 30)))


def scene_arrays(cfg):
    """(depth frames uint16, image frames uint8 x 3, the pixels (u, v) a tie byte was planted for)"""
    rng = np.random.default_rng(cfg["scene_seed"])
    rows, cols = cfg["rows"], cfg["cols"]
    deps, imgs, ties = [], [], []
    for holes in cfg["holes"]:
        d = rng.integers(2000, 12000, (rows, cols)) if cfg["depth_range"] == "near" else rng.integers(1, 65536, (rows, cols))
        d[rng.random((rows, cols)) < holes] = 0
        deps.append(d.astype(np.uint16))
    for colour in cfg["colour"]:
        if colour == "noise":
            im = rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8)
        elif colour == "constant":
            im = np.full((rows, cols, 3), int(rng.integers(0, 256)), np.uint8)
        else:
            im = np.zeros((rows, cols, 3), np.uint8)
            if rows >= 4 and cols >= 4:
                for (r, c) in TIE_WORDS.values():      # the low byte of patch word (r, c) of an inner pixel (u, v)
                    u, v = int(rng.integers(2, cols - 1)), int(rng.integers(2, rows - 1))
                    im[v - 1 + r].reshape(-1)[(u - 1) * 3 + 2 * c] = 1
                    ties.append((u, v))
        imgs.append(im)
    return deps, imgs, ties


def positions(rng, n, rows, cols, ties):
    """(n, 2) float32: integer pixels, sub-pixel positions, positions in (-1, 0), the last column and row, `cols` and `rows`
    themselves, the values no pixel can be taken from, and the pixels a tie was planted for"""
    kind = rng.choice(7, n, p=[0.3, 0.3, 0.06, 0.1, 0.08, 0.08, 0.08])
    xy = np.stack([rng.uniform(0, cols, n), rng.uniform(0, rows, n)], 1)
    whole = np.floor(xy)
    axis, both = rng.integers(0, 2, n), rng.random(n) < 0.3
    for i in range(n):
        k, a = kind[i], axis[i]
        if k == 0:
            xy[i] = whole[i]
        elif k == 2:
            xy[i, a] = -rng.uniform(0.001, 0.999)
        elif k == 3:
            xy[i, a] = (cols, rows)[a] - 1 + (rng.uniform(0, 0.999) if both[i] else 0.0)
        elif k == 4:
            xy[i, a] = (cols, rows)[a]
            if both[i]:
                xy[i, 1 - a] = (cols, rows)[1 - a]
        elif k == 5:
            xy[i, a] = SPECIALS[int(rng.integers(0, len(SPECIALS)))]
        elif k == 6:
            xy[i] = ties[int(rng.integers(0, len(ties)))] if ties else whole[i]
    return xy.astype(f32)


def depth_coordinates(rng, n):
    """(n, 3) float32 points whose z is a depth-range value, 0, NaN, negative or 1e30"""
    pts = rng.uniform(-3, 3, (n, 3))
    z = rng.uniform(0.2, 13.0, n)
    kind = rng.choice(5, n, p=[0.6, 0.1, 0.1, 0.1, 0.1])
    for k, v in ((1, 0.0), (2, np.nan), (3, -1.5), (4, 1e30)):
        z[kind == k] = v
    pts[:, 2] = z
    return pts.astype(f32)


def needs_images(model, outs):
    return "gradient" in outs or ("info" in outs and model == 2)


def scene_device(cfg, deps, imgs, with_images):
    """(geometry, sensor, the depth view, the image view or None) of the scene on the device, both blocks padded as drawn"""
    from putslam_amd._abi import frame_geometry, sensor_model
    ddep = strided_block(deps, cfg["depth_pad"][0], cfg["depth_pad"][1], PAD16)
    dimg = strided_block(imgs, cfg["image_pad"][0], cfg["image_pad"][1], PAD8) if with_images else None
    return frame_geometry(np.array(cfg["K"], f32), (0.0,) * 5, cfg["scale"]), sensor_model(**cfg["sensor"]), ddep, dimg


# ================================================================================================ uncertainty
UNC_CAPS = (1, 64, 257, 300)
UNC_COUNTS = (-1, 0, 1, 63, 64, 65, 255, 256, 257)
SUBSETS = [tuple(m for k, m in enumerate(MEMBERS) if bits >> k & 1) for bits in range(1, 8)]


def draw_uncertainty(rng):
    """A scene, F = 1 .. 4 row sets each naming a frame -- -1 and one past the depth set among them --, a capacity of 1, 64, 257 or
    300 (two blocks of 256 rows), counts on both sides of the wave and of the block, clipped to the capacity plus one; a model, a
    subset of the three outputs, and no image set where nothing needs one in half of those draws."""
    cfg = draw_scene(rng)
    F, cap = int(rng.integers(1, 5)), pick(rng, UNC_CAPS, (1, 2, 2, 3))
    D = cfg["depth_frames"]
    cfg.update(F=F, cap=cap, counts=[min(pick(rng, UNC_COUNTS + (cap, cap + 1), (1, 1, 1, 1, 1, 1, 1, 1, 1, 3, 1)), cap + 1) for _ in range(F)],
               image_frame=[pick(rng, list(range(D)) + [-1, D], [6] * D + [1, 2]) for _ in range(F)], outs=list(pick(rng, SUBSETS)),
               images_null=bool(rng.integers(0, 2)), rows_seed=int(rng.integers(0, 1 << 30)), redraws=0)
    return cfg


def images_passed(cfg):
    return needs_images(cfg["model"], cfg["outs"]) or not cfg["images_null"]


def uncertainty_inputs(cfg):
    """dict(deps, imgs, xy (F, cap, 2), pts (F, cap, 3)): every row of the capacity is a position, whatever the count"""
    deps, imgs, ties = scene_arrays(cfg)
    rng = np.random.default_rng(cfg["rows_seed"])
    F, cap = cfg["F"], cfg["cap"]
    xy = np.stack([positions(rng, cap, cfg["rows"], cfg["cols"], ties) for _ in range(F)])
    pts = np.stack([depth_coordinates(rng, cap) for _ in range(F)])
    return dict(deps=deps, imgs=imgs, xy=xy, pts=pts)


def uncertainty_reference(cfg, inputs=None, image_bound=True, variant=""):
    """Per set None (a count outside 0 .. cap: nothing is written) or uncertainty_ref.rows' dict of the wanted members.
    image_bound=False is the mutant that forgets `frame < iFrames`: it follows the frame into the last image there is; variant
    names a computation under a changed uncertainty_ref (another mutant), kept apart from the restatement's."""
    def compute():
        inp = inputs or uncertainty_inputs(cfg)
        s, K = U.sensor(**cfg["sensor"]), np.array(cfg["K"], f32)
        D, I, passed = cfg["depth_frames"], cfg["image_frames"], images_passed(cfg)
        out = []
        for f, (n, g) in enumerate(zip(cfg["counts"], cfg["image_frame"])):
            if not 0 <= n <= cfg["cap"]:
                out.append(None)
                continue
            inside = 0 <= g < D and (not passed or g < I or not image_bound)
            image = inp["imgs"][min(g, I - 1)] if inside and passed else None
            out.append(U.rows(inp["xy"][f, :n], inp["pts"][f, :n], inp["deps"][g] if inside else None, image, K, cfg["scale"], s, cfg["model"],
                              want=tuple(cfg["outs"])))
        return out
    return _memo("uncertainty" + variant + ("" if image_bound else " without the image bound"), cfg, compute)


def compare_uncertainty(ctx, cfg):
    import torch
    from putslam_amd import device_batch as D
    from putslam_amd._abi import PsUncertaintyOut
    why = Why()
    inp = uncertainty_inputs(cfg)
    want = uncertainty_reference(cfg, inp)
    F, cap = cfg["F"], cfg["cap"]
    geo, sens, ddep, dimg = scene_device(cfg, inp["deps"], inp["imgs"], images_passed(cfg))
    ds = D.DepthSet(ddep, cfg["rows"], cfg["cols"])
    iset = D._image_set(dimg, cfg["rows"], cfg["cols"], 3) if dimg is not None else None
    dxy, dpts = dev(inp["xy"]), dev(inp["pts"])
    dcnt, dfr = dev(np.array(cfg["counts"], np.int32)), dev(np.array(cfg["image_frame"], np.int32))
    out = {m: filled((F, cap, 9 if m == "info" else 3), f64) for m in MEMBERS}
    torch.cuda.synchronize()
    o = PsUncertaintyOut(*[out[m].data_ptr() if m in cfg["outs"] else None for m in MEMBERS])
    ctx.feature_uncertainty_device(geo, sens, cfg["model"], iset, ds, dfr.data_ptr(), dxy.data_ptr(), dpts.data_ptr(), dcnt.data_ptr(), F, cap, o)
    ctx.synchronize()
    for m in MEMBERS:
        got = out[m].cpu().numpy()
        if m not in cfg["outs"]:
            why.note(untouched(got), "an output that was not asked for", m)
            continue
        for f, w in enumerate(want):
            n = 0 if w is None else len(w[m])
            if n:
                bad = np.flatnonzero((got[f, :n].view(np.uint64) != w[m].view(np.uint64)).any(axis=1))
                why.note(len(bad) == 0, m, f, bad[:6].tolist(), [(inp["xy"][f, k].tolist(), got[f, k].tolist(), w[m][k].tolist()) for k in bad[:2]])
            why.note(untouched(got[f, n:]), m + " beyond its count", f)
    return why


def run_uncertainty(iters, seed, ctx=None, verbose=True):
    """ps_feature_uncertainty against uncertainty_ref.rows: the normal, the gradient and the information matrix of every row."""
    return _run("uncertainty", iters, seed, ctx, verbose, compare_uncertainty)


# ================================================================================================ edges
EDGE_MAX_MATCHES = (1, 63, 64, 255, 256, 257, 513, 640)
EDGE_TILE = 256                                     # ps_measurement_edges_rows compacts a pair's mask in tiles of this many bytes
EDGE_KPTS = (1, 16, 96)
EDGE_MASKS = ("empty", "full", "sparse", "last_tile")
EDGE_OUTPUTS = ("count", "map_row", "cur_row", "uv", "position") + MEMBERS
EDGE_NAMES = dict(map_row="mapRow", cur_row="curRow")
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def train_outside(max_kpts):
    return (-1, max_kpts, INT32_MIN, INT32_MAX)


def draw_edges(rng):
    """A scene; a map batch of 1 .. 2 views and 1 .. 3 frames of 1, 16 or 96 rows; P = 1 .. 8 pairs, some naming a view or a frame
    outside; lists of a drawn capacity with numMatches from the named values and from anywhere; per pair a mask that is empty,
    full, sparse or one inlier in the last tile, with the bytes beyond numMatches set in half the draws; in two draws of five some
    inliers' trainIdx lie outside the frame's rows; a subset of the eight outputs (each present three times in four; one draw in
    eight wants nothing but the count, one in sixteen nothing at all)."""
    cfg = draw_scene(rng)
    V, Fr, P, M = int(rng.integers(1, 3)), int(rng.integers(1, 4)), int(rng.integers(1, 9)), pick(rng, EDGE_MAX_MATCHES, (1, 1, 1, 1, 2, 2, 3, 3))
    D = cfg["depth_frames"]

    def pair():
        x = rng.random()
        view, fr = int(rng.integers(0, V)), int(rng.integers(0, Fr))
        return (pick(rng, (-1, V)), fr) if x < 0.06 else ((view, pick(rng, (-1, Fr))) if x < 0.12 else (view, fr))

    x = rng.random()
    outs = ["count"] if x < 0.125 else ([] if x < 0.1875 else [n for n in EDGE_OUTPUTS if rng.random() < 0.75])
    cfg.update(views=V, frames=Fr, max_kpts=pick(rng, EDGE_KPTS, (1, 2, 3)), max_matches=M, pairs=[pair() for _ in range(P)],
               num_matches=[pick(rng, (-300, 0, 1, M - 1, M, M + 1, int(rng.integers(1, M + 1))), (1, 1, 1, 2, 3, 1, 3)) for _ in range(P)],
               masks=[pick(rng, EDGE_MASKS, (1, 3, 3, 1)) for _ in range(P)], density=round(float(rng.uniform(0.02, 0.9)), 3),
               beyond=bool(rng.integers(0, 2)), bad_train=bool(rng.random() < 0.4), image_frame=[pick(rng, list(range(D)) + [-1, D], [6] * D + [1, 1]) for _ in range(Fr)],
               outs=outs, images_null=bool(rng.integers(0, 2)), rows_seed=int(rng.integers(0, 1 << 30)), redraws=0)
    return cfg


def edge_pair_valid(cfg, p):
    m, (view, fr) = cfg["num_matches"][p], cfg["pairs"][p]
    return 0 < m <= cfg["max_matches"] and 0 <= view < cfg["views"] and 0 <= fr < cfg["frames"]


def edges_inputs(cfg):
    """dict(deps, imgs, desc, pts (frames, max_kpts, 3), xyu (frames, max_kpts, 2), matches (P, max_matches) DMatch, mask, num,
    planted: [(pair, inlier number, trainIdx)] of the indices outside)"""
    from putslam_amd._abi import DMATCH_DTYPE
    deps, imgs, ties = scene_arrays(cfg)
    rng = np.random.default_rng(cfg["rows_seed"])
    Fr, cap, M, P = cfg["frames"], cfg["max_kpts"], cfg["max_matches"], len(cfg["pairs"])
    n_sets = max(Fr, cfg["views"])
    desc = rng.integers(0, 256, (n_sets, cap, 32)).astype(np.uint8)
    pts = np.stack([depth_coordinates(rng, cap) for _ in range(n_sets)])
    xyu = np.stack([positions(rng, cap, cfg["rows"], cfg["cols"], ties) for _ in range(Fr)])
    matches = np.zeros((P, M), DMATCH_DTYPE)
    matches["queryIdx"], matches["trainIdx"] = rng.integers(0, cap, (P, M)), rng.integers(0, cap, (P, M))
    matches["distance"] = rng.random((P, M)).astype(f32)
    mask, planted = np.zeros((P, M), np.uint8), []
    for p, kind in enumerate(cfg["masks"]):
        m = min(max(cfg["num_matches"][p], 0), M)
        if kind == "full":
            mask[p, :m] = 1
        elif kind == "sparse":
            mask[p, :m] = (rng.random(m) < cfg["density"]) * rng.choice((1, 2, 255), m)
        elif kind == "last_tile" and m:
            mask[p, int(rng.integers((m - 1) // EDGE_TILE * EDGE_TILE, m))] = 1
        if cfg["beyond"]:
            mask[p, m:] = 1                               # beyond numMatches: not read
        inl = np.flatnonzero(mask[p, :m])
        if cfg["bad_train"] and len(inl) and edge_pair_valid(cfg, p):
            at = rng.permutation(len(inl))[:4]
            for k, t in zip(at.tolist(), rng.permutation(train_outside(cap)).tolist()):
                matches["trainIdx"][p, inl[k]] = t
                planted.append((p, k, t))
    return dict(deps=deps, imgs=imgs, desc=desc, pts=pts, xyu=xyu, matches=matches, mask=mask, num=np.array(cfg["num_matches"], np.int32),
                planted=planted)


def edges_reference(cfg, inputs=None):
    """uncertainty_ref.measurement_edges' list of dicts per pair, with the members the draw wants"""
    def compute():
        inp = inputs or edges_inputs(cfg)
        images = inp["imgs"] if images_passed(cfg) else None
        return U.measurement_edges(inp["matches"], inp["num"], inp["mask"], cfg["pairs"], cfg["views"], inp["pts"][:cfg["frames"]], inp["xyu"],
                                   cfg["image_frame"], inp["deps"], images, np.array(cfg["K"], f32), cfg["scale"], U.sensor(**cfg["sensor"]),
                                   cfg["model"], cfg["max_matches"], want=tuple(m for m in MEMBERS if m in cfg["outs"]))
    return _memo("edges", cfg, compute)


def compare_edges(ctx, cfg):
    import torch
    from putslam_amd import device_batch as D
    why = Why()
    inp = edges_inputs(cfg)
    want = edges_reference(cfg, inp)
    P, M, V, Fr = len(cfg["pairs"]), cfg["max_matches"], cfg["views"], cfg["frames"]
    geo, sens, ddep, dimg = scene_device(cfg, inp["deps"], inp["imgs"], images_passed(cfg))
    cap = cfg["max_kpts"]
    level = np.zeros((max(V, Fr), cap), np.int32)
    batch = D.MapBatchDevice(D.FrameSetDevice(inp["desc"][:V], inp["pts"][:V], [cap] * V), level[:V],
                             D.FrameSetDevice(inp["desc"][:Fr], inp["pts"][:Fr], [cap] * Fr), level[:Fr], cfg["pairs"], M)
    batch.matches.copy_(dev(inp["matches"].view(np.uint8).reshape(P, M, 16)))
    batch.num_matches.copy_(dev(inp["num"]))
    batch.mask.copy_(dev(inp["mask"]))
    out = D.MeasurementEdges(P, M, "cuda:0", want=())
    kinds = {torch.int32: np.int32, torch.float32: f32, torch.float64: f64}
    out.count = filled((P,), np.int32) if "count" in cfg["outs"] else None
    for name, dt, tail in D._EDGE_ARRAYS:
        setattr(out, name, filled((P, M) + tail, kinds[dt]) if name in cfg["outs"] else None)
    torch.cuda.synchronize()
    D.measurement_edges(ctx, batch, dev(inp["xyu"]), geo, ddep, dimg, sens, cfg["model"], np.array(cfg["image_frame"], np.int32), out=out)
    torch.cuda.synchronize()
    got = {name: getattr(out, name).cpu().numpy() for name in cfg["outs"]}
    for p, w in enumerate(want):
        n = w["count"]
        if "count" in got:
            why.note(int(got["count"][p]) == n, "count", p, int(got["count"][p]), n)
        for name in cfg["outs"]:
            if name == "count":
                continue
            if n:
                expect = np.ascontiguousarray(w[EDGE_NAMES.get(name, name)]).astype(got[name].dtype, copy=False)
                ok = bits_equal(got[name][p, :n], expect.reshape(got[name][p, :n].shape))
                why.note(ok, name, p, [] if ok else np.flatnonzero((got[name][p, :n].reshape(n, -1) != expect.reshape(n, -1)).any(axis=1))[:6].tolist())
            why.note(untouched(got[name][p, n:]), name + " beyond its count", p)
    return why


def run_edges(iters, seed, ctx=None, verbose=True):
    """ps_measurement_edges on a hand-written result block against uncertainty_ref.measurement_edges: count, mapRow, curRow, uv,
    position and the three members of every final inlier, in match-list order."""
    return _run("edges", iters, seed, ctx, verbose, compare_edges)


# ================================================================================================ assemble
ASM_CAPS = (1, 64, 65, 300)
ASM_COUNTS = (0, 1, 63, 64, 65, -1)                # and the capacity and the capacity + 1
ASM_SIDE = ("xy", "xy_undist", "angle", "response", "octave", "src_idx", "det_dist")
ASM_COLUMNS = ("response", "angle", "octave")


def draw_assemble(rng):
    """F = 1 .. 5 frames of a capacity of 1, 64, 65 or 300 rows: ps_gather_keypoints by a drawn permutation and drawn counts, then
    ps_assemble_frames on what it wrote, by a kept_idx that is a permutation or a draw with repeats and counts of its own.  Depth
    frames of 8 .. 60 rows and cols in a padded block, read from a drawn first frame; a drawn camera (fx, fy above 0); no
    distortion, or |k1|, |k2| up to 0.3 and |p1|, |p2| up to 0.01; positions inside, on the borders, at cols and rows, outside."""
    F, cap = int(rng.integers(1, 6)), pick(rng, ASM_CAPS, (1, 2, 2, 3))
    rows, cols = int(rng.integers(8, 61)), int(rng.integers(8, 61))
    counts = lambda: [min(pick(rng, ASM_COUNTS + (cap, cap + 1), (1, 1, 1, 1, 1, 1, 3, 1)), cap + 1) for _ in range(F)]   # noqa: E731
    flt = lambda v: float(f32(v))   # noqa: E731
    dist = [0.0] * 5
    if rng.random() < 0.6:
        dist = [float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.01, 0.01)), float(rng.uniform(-0.01, 0.01)), 0.0]
    first = int(rng.integers(0, 3))
    return dict(F=F, cap=cap, rows=rows, cols=cols, gather_counts=counts(), counts=counts(), kept=pick(rng, ("permutation", "repeats")),
                columns=[c for c in ASM_COLUMNS if rng.random() < 0.7], first_depth_frame=first, depth_frames=first + F + int(rng.integers(0, 2)),
                depth_pad=(int(rng.integers(0, 8)), int(rng.integers(0, 41))),
                K=[flt(rng.uniform(5, 600)), 0.0, flt(rng.uniform(0, cols)), 0.0, flt(rng.uniform(5, 600)), flt(rng.uniform(0, rows)), 0.0, 0.0, 1.0],
                dist5=dist, scale=pick(rng, (5000.0, 1000.0, 1.0)), seed=int(rng.integers(0, 1 << 30)), redraws=0)


def assemble_positions(rng, n, rows, cols):
    """(n, 2) float32: inside, on the borders, within half a pixel of cols and rows (the next-row read), outside"""
    xy = np.stack([rng.uniform(0, cols - 1, n), rng.uniform(0, rows - 1, n)], 1)
    kind = rng.choice(5, n, p=[0.45, 0.15, 0.2, 0.15, 0.05])
    axis = rng.integers(0, 2, n)
    for i in range(n):
        k, a = kind[i], axis[i]
        if k == 1:
            xy[i, a] = (0.0, (cols, rows)[a] - 1.0)[int(rng.integers(0, 2))]
        elif k == 2:
            xy[i, a] = (cols, rows)[a] - rng.uniform(0.0, 0.5)
        elif k == 3:
            xy[i] = (rng.uniform(-10, cols + 10), rng.uniform(-10, rows + 10))
        elif k == 4:
            xy[i, a] = (np.nan, np.inf, -np.inf, 1e30)[int(rng.integers(0, 4))]
    return xy.astype(f32)


def assemble_inputs(cfg):
    """dict(deps, xy (F, cap, 2), response, angle, octave (F, cap), idx: the gather's lists, kept: the assembly's)"""
    rng = np.random.default_rng(cfg["seed"])
    F, cap, rows, cols = cfg["F"], cfg["cap"], cfg["rows"], cfg["cols"]
    deps = []
    for _ in range(cfg["depth_frames"]):
        d = rng.integers(500, 20000, (rows, cols))
        d[rng.random((rows, cols)) < 0.15] = 0
        deps.append(d.astype(np.uint16))
    xy = np.stack([assemble_positions(rng, cap, rows, cols) for _ in range(F)])
    idx = np.stack([rng.permutation(cap) for _ in range(F)]).astype(np.int32)
    kept = idx[::-1].copy() if cfg["kept"] == "permutation" else rng.integers(0, cap, (F, cap)).astype(np.int32)
    return dict(deps=deps, xy=xy, response=rng.normal(size=(F, cap)).astype(f32), angle=rng.uniform(0, 360, (F, cap)).astype(f32),
                octave=rng.integers(0, 8, (F, cap)).astype(np.int32), idx=idx, kept=kept)


def gather_reference(cfg, inp):
    """(the gathered blocks xy, response, angle, octave -- sentinels beyond a count --, counts: -1 where a count lies outside)"""
    F, cap = cfg["F"], cfg["cap"]
    out = dict(xy=filled_host((F, cap, 2), f32), response=filled_host((F, cap), f32), angle=filled_host((F, cap), f32), octave=filled_host((F, cap), np.int32))
    counts = []
    for f, n in enumerate(cfg["gather_counts"]):
        counts.append(n if 0 <= n <= cap else -1)
        for name, block in out.items():
            if counts[-1] > 0:
                block[f, :n] = inp[name][f][inp["idx"][f, :n]]
    return out, counts


def assemble_reference(cfg, oracle, inputs=None):
    """(gather_reference's pair, per frame None or frame_assembly_ref.assemble's dict on the gathered rows)"""
    def compute():
        inp = inputs or assemble_inputs(cfg)
        g, gcounts = gather_reference(cfg, inp)
        frames = []
        for f, n in enumerate(cfg["counts"]):
            if not 0 <= n <= cfg["cap"]:
                frames.append(None)
                continue
            frames.append(A.assemble(oracle, g["xy"][f], inp["kept"][f, :n], inp["deps"][cfg["first_depth_frame"] + f], np.array(cfg["K"], f32),
                                     cfg["dist5"], cfg["scale"], **{c: g[c][f] for c in cfg["columns"]}))
        return (g, gcounts), frames
    return _memo("assemble", cfg, compute)


def _oracle():
    from oracle import oracle_py
    oracle_py.build()
    return oracle_py


def compare_assemble(ctx, cfg, oracle=None):
    import torch
    from putslam_amd import device_batch as D
    from putslam_amd._abi import frame_geometry
    why = Why()
    inp = assemble_inputs(cfg)
    (g, gcounts), frames = assemble_reference(cfg, oracle or _oracle(), inp)
    F, cap = cfg["F"], cfg["cap"]
    names = ["xy"] + [c for c in ASM_COLUMNS if c in cfg["columns"]]
    kinds = dict(xy=f32, response=f32, angle=f32, octave=np.int32)
    ins = {n: dev(inp[n]) for n in names}
    outs = {n: filled((F, cap, 2) if n == "xy" else (F, cap), kinds[n]) for n in names}
    cnt = filled((F,), np.int32)
    ptr = lambda d, n: d[n].data_ptr() if n in d else 0   # noqa: E731
    di, dn = dev(inp["idx"]), dev(np.array(cfg["gather_counts"], np.int32))
    torch.cuda.synchronize()
    ctx.gather_keypoints(di.data_ptr(), dn.data_ptr(), F, cap, *[ptr(ins, n) for n in ("xy",) + ASM_COLUMNS], *[ptr(outs, n) for n in ("xy",) + ASM_COLUMNS],
                         cnt.data_ptr())
    ctx.synchronize()
    why.note(cnt.cpu().numpy().tolist() == gcounts, "gather counts", cnt.cpu().numpy().tolist(), gcounts)
    for n in names:
        why.note(bits_equal(outs[n].cpu().numpy(), g[n]), "gather", n)
    # the assembly on the gathered blocks where they lie
    side = [s for s in ASM_SIDE if s not in ASM_COLUMNS or s in cfg["columns"]]
    out = D.FrameRowsDevice(F, cap, "cuda:0", side)
    rows_kinds = {torch.float32: f32, torch.int32: np.int32, torch.float64: f64}
    for name in ["pts", "nkpts"] + side:
        t = getattr(out, name)
        setattr(out, name, filled(tuple(t.shape), rows_kinds[t.dtype]))
    ddep = strided_block(inp["deps"], cfg["depth_pad"][0], cfg["depth_pad"][1], PAD16)
    geo = frame_geometry(np.array(cfg["K"], f32), cfg["dist5"], cfg["scale"])
    torch.cuda.synchronize()
    D.assemble_frames(ctx, geo, ddep, outs["xy"], dev(inp["kept"]), dev(np.array(cfg["counts"], np.int32)), outs.get("angle"), outs.get("response"),
                      outs.get("octave"), first_depth_frame=cfg["first_depth_frame"], side=side, out=out)
    torch.cuda.synchronize()
    got = {name: getattr(out, name).cpu().numpy() for name in ["pts", "nkpts"] + side}
    why.note(got["nkpts"].tolist() == [0 if w is None else len(w["pts"]) for w in frames], "nkpts", got["nkpts"].tolist())
    for f, w in enumerate(frames):
        n = 0 if w is None else len(w["pts"])
        for name in ["pts"] + side:
            if n:
                why.note(same_words(got[name][f, :n], np.asarray(w[name]).astype(got[name].dtype)), name, f)
            why.note(untouched(got[name][f, n:]), name + " beyond its count", f)
    return why


def run_assemble(iters, seed, ctx=None, verbose=True, oracle=None):
    """ps_gather_keypoints against numpy's gather, then ps_assemble_frames on its blocks against frame_assembly_ref.assemble (the
    oracle's undistortion and back-projection)."""
    oracle = oracle or _oracle()
    return _run("assemble", iters, seed, ctx, verbose, lambda c, cfg: compare_assemble(c, cfg, oracle))


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
    bad, t0 = 0, time.time()
    for family in (FAMILIES if a.family == "all" else (a.family,)):
        n = globals()["run_" + family](a.iters, a.seed, ctx=ctx)      # (an exception -- a HIP error -- ends everything here)
        print(f"fuzz done: {family}, {a.iters} draws, {n} mismatches, {time.time() - t0:.0f} s since the start", flush=True)
        bad += n
    ctx.close()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
