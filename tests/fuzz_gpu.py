#!/usr/bin/env python3
"""Randomised soak test: HIP path vs oracle over many random configurations (sizes, inlier ratios, noise,
error modes, estimators, thresholds, seeds).  tests/test_gpu_fuzz_slice.py collects a 300-configuration slice under
`-m gpu`; longer soaks are run by hand on the GPU box:

    python tests/fuzz_gpu.py --iters 3000 --seed 1
    python tests/fuzz_gpu.py --iters 100000 --procs 8 --modes 0,2,4 --counts     (round 3: the new scoring kernels)
    python tests/fuzz_gpu.py --batch --iters 400 --procs 4                       (staged scoring: random batches)
    python tests/fuzz_gpu.py --map --iters 2000 --procs 4                        (guided map matching: random device batches)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import oracle_py as po  # noqa: E402
from putslam_amd import api, synth  # noqa: E402
from putslam_amd._abi import EST_FIXED, EST_RANSAC, EST_USAC, TUM_FR1_K, default_ransac_params, make_config  # noqa: E402


def run(iters, seed, max_kpts=1500, ctx=None, verbose=True, modes=(0, 1, 2, 4, 3), counts=False):
    """Returns the number of configurations in which the HIP path and the oracle disagree.  counts=True also compares
    the inlier count of EVERY hypothesis (ps_debug_ransac_counts vs po_hypothesis_counts), not only the call's outputs."""
    rng = np.random.default_rng(seed)
    ctx = ctx or api.Context(0)
    t0 = time.time()
    bad = 0
    for it in range(iters):
        n = int(rng.integers(4, max_kpts))
        frac = float(rng.uniform(0.05, 0.95))
        noise = float(10 ** rng.uniform(-4, -1.3))
        pa, pb = synth.make_pair(n, config=7, index=int(rng.integers(0, 2 ** 31)), inlier_frac=frac, noise=noise)
        mode = int(rng.choice(list(modes)))
        # (RANSAC: the reference's 1157 -- the schedule never needs more than 574 with the default ratios -- or a cap of at most
        # 520: kernel 4 replays schedules of up to 512 iterations per wavefront out of registers, longer ones as a work-group)
        est, H = [(EST_RANSAC, [1157, 487, int(rng.integers(1, 520))][int(rng.integers(0, 3))]),
                  (EST_USAC, int(rng.integers(50, 3000))), (EST_FIXED, int(rng.integers(1, 3000)))][int(rng.integers(0, 3))]
        if est == EST_RANSAC and n <= 150 and rng.random() < 0.3:
            # long RANSAC caps: with minimalInlierRatioThreshold = 0.05 the schedule may run for 31 294 iterations (a stop table
            # of that many floats, the work-group replay, stage 1 walked by looping work-groups)
            H = int(rng.integers(2000, 60000))
        if est == EST_USAC and n <= 150 and rng.random() < 0.3:
            # long schedules (the reference's cap is 850 000): few matches keep the oracle's loop affordable; the stop table has
            # one entry per hypothesis and the work-group replay walks all of its search windows
            H = int(rng.integers(100000, 850001))
        prm = default_ransac_params(mode, lc=bool(rng.integers(0, 2)))
        prm.inlierThresholdEuclidean = float(10 ** rng.uniform(-3, -0.5))
        prm.inlierThresholdReprojection = float(10 ** rng.uniform(-1, 1.5))
        prm.minimalInlierRatioThreshold = float(rng.choice([0.05, 0.1, 0.15, 0.2, 0.3, 0.5]))
        prm.minimalNumberOfMatches = int(rng.choice([3, 8, 10, 15, 40]))
        K = TUM_FR1_K if rng.random() < 0.9 else TUM_FR1_K * np.float32(10 ** rng.uniform(-3, 3))
        cfg, _ = make_config(est, H, seed=int(rng.integers(0, 2 ** 62)))
        mg = ctx.match_hamming256(pa["desc"], pb["desc"])
        mc = po.match_hamming256(pa["desc"], pb["desc"])
        ok = mg.tobytes() == mc.tobytes()
        g = ctx.ransac_rigid3d(prm, cfg, K, pa["pts"], pb["pts"], mc)
        c = po.ransac_rigid3d(prm, cfg, K, pa["pts"], pb["pts"], mc)
        ok &= np.array_equal(g["mask"], c["mask"]) and g["pose"].tobytes() == c["pose"].tobytes()
        for f in c["stats"].dtype.names:
            x, y = g["stats"][f], c["stats"][f]
            ok &= bool(x == y or (np.isnan(x) and np.isnan(y)))
        if counts:
            # (the scoring kernels do not run below the schedule's minimum number of matches -- RANSAC.cpp:77-80,
            # USAC_wrapper.cpp:120 -- and the diagnostic then returns zeros; the oracle's count function has no such gate)
            min_run = max(3, 8 if est == EST_USAC else int(prm.minimalNumberOfMatches))
            if int(c["stats"]["numMatchesValid"]) >= min_run:
                cg = ctx.debug_ransac_counts(prm, cfg, K, pa["pts"], pb["pts"], mc)
                cc, _ = po.hypothesis_counts(prm, cfg, K, pa["pts"], pb["pts"], mc)
                ok &= np.array_equal(cg, cc[: len(cg)])
        if not ok:
            bad += 1
            print("MISMATCH", dict(it=it, n=n, frac=frac, noise=noise, mode=mode, est=est, H=H), g["stats"], c["stats"], flush=True)
        if verbose and (it + 1) % 200 == 0:
            print(f"{it + 1} iterations, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
    return bad


STAT_FIELDS = ("numMatchesIn", "numMatchesValid", "bestHypothesis", "bestInlierCount", "iterationsRun", "numInliers",
               "accepted", "bestInlierRatio", "pointInlierRatio")


def run_batch(iters, seed, verbose=True, modes=(0, 1, 2, 4), oracle_pairs=3):
    """Random BATCHES large enough for the staged scoring (ps_score_pass.h): the staged run with the reordered match record
    (options prune = 1, reorder = 1) against the staged run in the original order (reorder = 0) and the complete one
    (prune = 0: the launch form the single-pair soak above checks against the oracle) on every pair and every output
    field, and against the oracle on a few pairs of each batch.  Returns the number of batches with a difference."""
    from putslam_amd.device_batch import FrameSetDevice, PairBatchDevice, run_pairs
    rng = np.random.default_rng(seed)
    t0 = time.time()
    bad = 0
    ctxs = {}
    for pr in (1, 2, 0):   # 1: staged, reordered match record; 2: staged, original order; 0: complete
        ctxs[pr] = api.Context(0)
        ctxs[pr].set_option("prune", 2 if pr else 0)   # (2: staged whatever the batch size; the default asks the cost model)
        ctxs[pr].set_option("reorder", 1 if pr == 1 else 0)
    for it in range(iters):
        mode = int(rng.choice(list(modes)))
        est, H = [(EST_RANSAC, int(rng.choice([487, 1157, 2000]))), (EST_USAC, int(rng.integers(300, 5000))),
                  (EST_FIXED, int(rng.integers(257, 6000)))][int(rng.integers(0, 3))]
        long_usac = est == EST_USAC and rng.random() < 0.08
        if long_usac:  # caps up to the reference's 850 000: one stop-table entry per hypothesis, survivor lists of that length
            H = int(rng.integers(100000, 850001))
        if est == EST_FIXED and rng.random() < 0.08:  # many hypotheses, few pairs: long survivor lists, list stages in several passes
            H = int(rng.integers(20000, 120001))
            long_usac = True  # (the same shape of batch: few small frames)
        hb = (H + 255) // 256
        kpts = int(rng.integers(40, 300 if long_usac else 900))
        # (staged from P (hb - 1) >= 256 (Euclidean kernels) / 768 (reprojection kernels) on: most batches are above)
        frames = int(max(6, min(400, 800 // max(hb - 1, 1) + int(rng.integers(2, 60)))))
        if long_usac:
            frames = int(rng.integers(3, 9))  # (the oracle walks the schedule hypothesis by hypothesis)
        frac = float(rng.uniform(0.05, 0.95))
        noise = float(10 ** rng.uniform(-4, -1.5))
        seq = synth.make_sequence(frames, kpts, config=3, index=int(rng.integers(0, 2 ** 31)), inlier_frac=frac, noise=noise)
        if rng.random() < 0.3:  # ragged keypoint counts, a few nearly empty frames
            for f in rng.integers(0, frames, max(1, frames // 8)):
                seq["nkpts"][f] = int(rng.integers(0, kpts))
        if rng.random() < 0.2:  # quantised points: groups of bit-identical models and counts (ties)
            seq["pts"] = (np.round(seq["pts"] * 64) / 64).astype(np.float32)
        prm = default_ransac_params(mode, lc=bool(rng.integers(0, 2)))
        prm.inlierThresholdEuclidean = float(10 ** rng.uniform(-2.5, -0.7))
        prm.inlierThresholdReprojection = float(10 ** rng.uniform(-0.5, 1.2))
        prm.minimalInlierRatioThreshold = float(rng.choice([0.02, 0.05, 0.1, 0.2, 0.3]))
        base = int(rng.integers(0, 2 ** 40))
        cfg, _ = make_config(est, H, seed=base)
        outs = {}
        for pr in (1, 2, 0):
            fs = FrameSetDevice(seq["desc"], seq["pts"], seq["nkpts"])
            pb = PairBatchDevice(seq["pairs"], fs.max_kpts)
            run_pairs(ctxs[pr], prm, cfg, TUM_FR1_K, fs, pb)
            outs[pr] = pb.download()
            if hasattr(ctxs[pr], "debug_keys_clean") and it % 8 == 0:
                # the matcher's atomicMin merge starts from an all-ones keys block that kernel 2 restores (no clearing launch)
                assert ctxs[pr].debug_keys_clean() == 0, ("keys block not all-ones at rest", it, pr)
        a = outs[1]
        P = len(seq["pairs"])
        why = []   # what differs, for the log: (against what, pair, field)

        def note(cond, *what):
            if not cond and len(why) < 12:
                why.append(what)
            return bool(cond)

        ok = True
        for tag, b in (("staged/original order", outs[2]), ("complete", outs[0])):
            ok &= note(np.array_equal(a["numMatches"], b["numMatches"]), tag, "numMatches")
            for p in range(P):
                n = int(a["numMatches"][p])
                ok &= note(a["pose"][p].tobytes() == b["pose"][p].tobytes(), tag, p, "pose")
                ok &= note(np.array_equal(a["inlierMask"][p, :n], b["inlierMask"][p, :n]), tag, p, "mask")
                for f in STAT_FIELDS:
                    x, y = a["stats"][p][f], b["stats"][p][f]
                    ok &= note(bool(x == y or (np.isnan(x) and np.isnan(y))), tag, p, f, x, y)
        for p in rng.integers(0, P, oracle_pairs):
            cfgp, _ = make_config(est, H, seed=base + int(p))
            c = po.vo_pairs(prm, cfgp, TUM_FR1_K, seq["desc"], seq["pts"], seq["nkpts"], seq["pairs"][p:p + 1], threads=1)
            n = int(c["numMatches"][0])
            ok &= note(n == int(a["numMatches"][p]) and np.array_equal(a["inlierMask"][p, :n], c["inlierMask"][0, :n]), "oracle", int(p), "mask")
            ok &= note(a["pose"][p].tobytes() == c["pose"][0].tobytes(), "oracle", int(p), "pose")
            for f in STAT_FIELDS:
                x, y = a["stats"][p][f], c["stats"][0][f]
                ok &= note(bool(x == y or (np.isnan(x) and np.isnan(y))), "oracle", int(p), f, x, y)
        if not ok:
            bad += 1
            print("MISMATCH", dict(it=it, mode=mode, est=est, H=H, frames=frames, kpts=kpts, frac=frac, noise=noise, seed=base),
                  "differences:", why, flush=True)
        if verbose and (it + 1) % 20 == 0:
            print(f"{it + 1} batches, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
    for c in ctxs.values():
        c.close()
    return bad


MAP_WIDTHS = (20, 64, 65, 128)


def draw_map(rng):
    """One configuration of run_map (no GPU): ragged views and frames of capacity <= 600 (tests/match_xyz_model_f64.py's
    generators), binary rows or float rows of a width of MAP_WIDTHS, dense or pitched, P pairs in 1 .. 80 (a few of them naming a
    view or a frame outside its set), radius from the retry ladder or log-uniform in [0.03, 1], ratio in [0.1, 0.9], both scalar or
    per pair."""
    import match_xyz_model_f64 as model
    kind = "binary" if rng.random() < 0.4 else int(rng.choice(MAP_WIDTHS))

    def ragged(n, cap):
        out = []
        for _ in range(n):
            x = rng.random()
            out.append(0 if x < 0.12 else 1 if x < 0.2 else cap if x < 0.35 else int(rng.integers(0, cap + 1)))
        return out

    vcap, fcap = (int(round(10 ** rng.uniform(0.5, np.log10(600)))) for _ in range(2))
    V, F = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    source = rng.integers(0, F, V)
    views, frames = model.sets(rng, ragged(V, vcap), ragged(F, fcap), vcap, fcap, source, kind)
    P = int(rng.integers(1, 81))
    pairs = np.zeros((P, 2), np.int32)
    for p in range(P):
        v = int(rng.integers(0, V))
        pairs[p] = (v, source[v] if rng.random() < 0.7 else rng.integers(0, F))
        if rng.random() < 0.03:
            col = int(rng.integers(0, 2))
            pairs[p, col] = [-1, (V, F)[col], 1000][int(rng.integers(0, 3))]
    n = P if rng.random() < 0.5 else 1
    radius = [model.ladder(0.12, 0.55, int(rng.integers(1, 11)))[0] if rng.random() < 0.5 else float(10 ** rng.uniform(np.log10(0.03), 0))
              for _ in range(n)]
    ratio = [float(rng.uniform(0.1, 0.9)) for _ in range(n)]
    return dict(kind=kind, views=views, frames=frames, pairs=pairs, radius=radius if n > 1 else radius[0],
                ratio=ratio if n > 1 else ratio[0], pitched=bool(rng.random() < 0.5), short=bool(rng.random() < 0.35),
                cut=float(rng.uniform(0.2, 0.95)), pad=int(rng.choice([1, 4, 12])))


def map_answers(cfg):
    """Per pair of a draw_map configuration: (the match list of oracle.match_xyz / map_l2_ref.match_xyz_l2, the model's
    Answer), each computed once per distinct (view, frame, radius, ratio)."""
    import map_l2_ref
    import match_xyz_model_f64 as model
    from putslam_amd._abi import DMATCH_DTYPE
    views, frames = cfg["views"], cfg["frames"]
    done, out = {}, []
    for p, (v, f) in enumerate(cfg["pairs"]):
        r = cfg["radius"][p] if np.ndim(cfg["radius"]) else cfg["radius"]
        a = cfg["ratio"][p] if np.ndim(cfg["ratio"]) else cfg["ratio"]
        key = (int(v), int(f), r, a)
        if key not in done:
            if not (0 <= v < len(views["nkpts"]) and 0 <= f < len(frames["nkpts"])):
                done[key] = (np.zeros(0, DMATCH_DTYPE), model.Answer(0, cfg["kind"] != "binary"))
            else:
                sides = model.side(views, v) + model.side(frames, f)
                if len(sides[0]) == 0 or len(sides[3]) == 0:
                    m = np.zeros(0, DMATCH_DTYPE)
                else:
                    m = (po.match_xyz if cfg["kind"] == "binary" else map_l2_ref.match_xyz_l2)(*sides, r, a)
                done[key] = (m, model.match_xyz(*sides, r, a))
        out.append(done[key])
    return out


def map_max_matches(cfg, answers):
    """The rows per pair: the largest count, or (cfg short) a part of it, so that some pairs report -(count)."""
    top = max([len(m) for m, _ in answers] + [1])
    return max(1, int(top * cfg["cut"])) if cfg["short"] else top


def map_model_failures(answers, lists=None):
    """The shared check of every pair's list (default: the CPU answer's own) against the model, the cap on ambiguous features
    taken over the whole configuration (one scene).  Returns the failures."""
    import match_xyz_model_f64 as model
    fails, amb, cand = [], 0, 0
    seen = set()
    for p, (m, ans) in enumerate(answers):
        got = m if lists is None else lists[p]
        if got is None:
            continue
        r = model.compare(got, ans)
        if id(ans) not in seen:
            seen.add(id(ans))
            amb, cand = amb + r.ambiguous, cand + r.with_candidates
        r.ambiguous = r.with_candidates = 0
        fails += [(p, x) for x in r.failures()]
    if amb > model.AMBIGUOUS_CAP * cand:
        fails.append(("cap", amb, cand))
    return fails


def run_map(iters, seed, ctx=None, verbose=True):
    """Random device batches of the guided map matching (ps_match_xyz_device / ps_match_xyz_l2_device): every pair's count and
    rows against oracle.match_xyz / map_l2_ref.match_xyz_l2 as bytes -- a pair whose count exceeds maxMatches reports -(count) --
    and through the shared check against the float64 model of tests/match_xyz_model_f64.py.  Returns the number of
    configurations with a difference."""
    from putslam_amd.device_batch import (FrameSetDevice, FrameSetF32Device, MapBatchDevice, MapBatchF32Device, PackedFrameSetDevice,
                                          run_match_xyz, run_match_xyz_l2)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(seed)
    ctx = ctx or api.Context(0)
    t0 = time.time()
    bad = 0
    for it in range(iters):
        cfg = draw_map(rng)
        views, frames, pairs = cfg["views"], cfg["frames"], cfg["pairs"]
        answers = map_answers(cfg)
        cap = map_max_matches(cfg, answers)
        if cfg["kind"] == "binary":
            if cfg["pitched"]:
                vs = PackedFrameSetDevice(views["desc"], views["pos"], views["nkpts"], stride=(views["cap"] * 44 + 15) // 16 * 16 + 16 * cfg["pad"])
                fs = PackedFrameSetDevice(frames["desc"], frames["pos"], frames["nkpts"])
            else:
                vs = FrameSetDevice(views["desc"], views["pos"], views["nkpts"])
                fs = FrameSetDevice(frames["desc"], frames["pos"], frames["nkpts"])
            b = MapBatchDevice(vs, views["level"], fs, frames["level"], pairs, cap, radius=cfg["radius"], ratio=cfg["ratio"])
            run_match_xyz(ctx, b)
        else:
            rf = cfg["kind"] + cfg["pad"] if cfg["pitched"] else None
            vs = FrameSetF32Device(views["desc"], views["pos"], views["nkpts"], row_floats=rf)
            fs = FrameSetF32Device(frames["desc"], frames["pos"], frames["nkpts"], row_floats=rf)
            b = MapBatchF32Device(vs, views["level"], fs, frames["level"], pairs, cap, radius=cfg["radius"], ratio=cfg["ratio"])
            run_match_xyz_l2(ctx, b)
        g = b.download()
        why, lists = [], []
        for p, (m, _) in enumerate(answers):
            n = int(g["numMatches"][p])
            if len(m) > cap:
                lists.append(None)
                if n != -len(m):
                    why.append((p, "count over capacity", n, -len(m)))
                continue
            lists.append(g["matches"][p, :max(n, 0)])
            if n != len(m) or lists[-1].tobytes() != m.tobytes():
                why.append((p, "bytes", n, len(m)))
        why += map_model_failures(answers, lists)
        if why:
            bad += 1
            print("MISMATCH", dict(it=it, seed=seed, kind=cfg["kind"], P=len(pairs), views=views["nkpts"].tolist(),
                                   frames=frames["nkpts"].tolist(), pitched=cfg["pitched"], cap=cap), "differences:", why[:12], flush=True)
        if verbose and (it + 1) % 20 == 0:
            print(f"{it + 1} map configurations, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
    return bad


def main():
    import faulthandler
    faulthandler.enable()   # a worker that dies on a signal leaves its Python stack in its log
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-kpts", type=int, default=1500)
    ap.add_argument("--modes", default="0,1,2,4,3", help="RANSAC::ERROR_VERSION values to draw from")
    ap.add_argument("--counts", action="store_true", help="also compare every hypothesis's inlier count")
    ap.add_argument("--procs", type=int, default=1, help="worker processes (seeds seed, seed+1, ...), iterations split evenly")
    ap.add_argument("--batch", action="store_true", help="random batches: staged scoring vs complete scoring vs oracle")
    ap.add_argument("--map", action="store_true", help="random device batches of the guided map matching vs oracle and float64 model")
    ap.add_argument("--log-dir", default=None,
                    help="where every worker's FULL output is kept (default: gpurun_out/fuzz_logs under the repository)")
    ap.add_argument("--tag", default="", help="label for the log files of this run")
    a = ap.parse_args()
    modes = tuple(int(x) for x in a.modes.split(","))
    if a.procs > 1:
        import subprocess
        po.lib()  # (build the oracle once, before the workers start)
        per = (a.iters + a.procs - 1) // a.procs
        log_dir = a.log_dir or os.path.join(ROOT, "gpurun_out", "fuzz_logs")
        os.makedirs(log_dir, exist_ok=True)
        stamp = f"{a.tag or 'run'}_{'map' if a.map else 'batch' if a.batch else 'single'}_{int(time.time())}_{os.getpid()}"
        ps, logs = [], []
        for i in range(a.procs):
            # every worker's complete output goes to a file of its own (round 3 lost the only failing worker's output to a
            # `tail -1`): nothing a worker printed before it died can be lost, whatever the caller does with this
            # process's stdout
            path = os.path.join(log_dir, f"{stamp}_worker{i}_seed{a.seed + i}.log")
            f = open(path, "w")
            logs.append((path, f))
            ps.append(subprocess.Popen([sys.executable, "-u", os.path.abspath(__file__), "--iters", str(per), "--seed", str(a.seed + i),
                                        "--max-kpts", str(a.max_kpts), "--modes", a.modes] + (["--counts"] if a.counts else [])
                                       + (["--batch"] if a.batch else []) + (["--map"] if a.map else []), stdout=f, stderr=subprocess.STDOUT, text=True))
        failed = 0
        for i, p in enumerate(ps):
            p.wait()
            path, f = logs[i]
            f.close()
            out = open(path).read()
            lines = out.splitlines()
            tail = [l for l in lines if l.startswith("fuzz done") or l.startswith("MISMATCH")]
            print(f"[worker {i}, seed {a.seed + i}, rc {p.returncode}] " + " | ".join(tail[-4:]), flush=True)
            finished = any(l.startswith("fuzz done") for l in lines)
            if p.returncode != 0 or not finished:
                failed += 1
                # ANY non-zero exit or missing summary line fails the run and is shown in full (last 60 lines), whether it was a
                # mismatch, a Python exception, a HIP error or a signal (negative return code)
                kind = "MISMATCH" if any(l.startswith("MISMATCH") for l in lines) else \
                    (f"killed by signal {-p.returncode}" if p.returncode < 0 else "died")
                print(f"[worker {i}] {kind}: exit code {p.returncode}, full log kept at {path}; last output:\n  "
                      + "\n  ".join(lines[-60:]), flush=True)
        print(f"fuzz done: {per * a.procs} iterations over {a.procs} workers, modes {a.modes}, "
              f"{'no mismatches' if failed == 0 else f'{failed} WORKER(S) FAILED (MISMATCHES or crashes, see above)'}")
        return 1 if failed else 0
    if a.map:
        bad = run_map(a.iters, a.seed)
    elif a.batch:
        bad = run_batch(a.iters, a.seed, modes=tuple(m for m in modes if m != 3))
    else:
        bad = run(a.iters, a.seed, a.max_kpts, modes=modes, counts=a.counts)
    print(f"fuzz done: {a.iters} iterations, {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
