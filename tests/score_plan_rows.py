"""What the host test of the scoring plan (tests/test_score_plan_host.py), the GPU tests of the cost model (tests/test_gpu_prune.py)
and the fixture's recipe (tests/golden/make_score_plan_parent.py) share: the cost model's rows, and the line format in which
tests/cpp/test_score_plan.cpp takes input tuples and prints what putslam_amd/csrc/ps_score_plan.h decides for them."""

# PsErrorVersion / PsEstimator (include/putslam_hip.h)
EUCLIDEAN_ERROR, REPROJECTION_ERROR, EUCLIDEAN_AND_REPROJECTION_ERROR, MAHALANOBIS_ERROR, ADAPTIVE_ERROR = 0, 1, 2, 3, 4
EST_RANSAC, EST_USAC, EST_FIXED = 0, 1, 2
VALUE, EUCLID, REPROJ = 0, 1, 2          # Scoring (ps_score_plan.h)
PS_OK, PS_ERR_UNSUPPORTED = 0, -5
K_STAGES = 3


def family_of(mode):
    """make_plan's choice with the decision-exact kernels on (option "score" = 1, the default)."""
    return {EUCLIDEAN_ERROR: EUCLID, ADAPTIVE_ERROR: EUCLID, REPROJECTION_ERROR: REPROJ, EUCLIDEAN_AND_REPROJECTION_ERROR: REPROJ}.get(mode, VALUE)


# (mode, est, H, kpts, below, above): threshold = base + perRow x capacity in units of pairs x (ceil(H / 256) - 1) x capacity
# (ps_score_plan.h: kStagedFrom); complete scoring with `below` pairs, the staged form with `above`
COST_MODEL_ROWS = [
    (EUCLIDEAN_ERROR, EST_FIXED, 4096, 500, 100, 140),       # 7.8e5 + 250 x 500 = 9.05e5: 121 pairs
    (REPROJECTION_ERROR, EST_FIXED, 4096, 400, 230, 270),    # 1.3e6 + 500 x 400 = 1.5e6: 250 pairs
    (EUCLIDEAN_ERROR, EST_RANSAC, 1157, 300, 40, 60),        # 6.0e4: 50 pairs (hb - 1 = 4)
    (REPROJECTION_ERROR, EST_USAC, 3000, 300, 10, 18),       # 4.5e4: 14 pairs (hb - 1 = 11)
]

# (mode, est, H, kpts, sbs, below, above): a context that shares the chip with other launch chains (option "side_by_side": the chains of
# a PsBatchQueue, the lanes of the pipelined stream) takes the staged form from far smaller batches on (ps_score_plan.h: kStagedFrom,
# side by side); with TWO chains the point lies half way, on the logarithmic scale
COST_MODEL_SBS_ROWS = [
    (EUCLIDEAN_ERROR, EST_FIXED, 4096, 500, 4, 56, 74),      # 4.5e5 + 75 x 500 = 4.875e5: 65 pairs (alone: 121)
    (REPROJECTION_ERROR, EST_FIXED, 4096, 400, 4, 48, 64),   # 3.0e5 + 90 x 400 = 3.36e5: 56 pairs (alone: 250)
    (REPROJECTION_ERROR, EST_FIXED, 4096, 400, 2, 104, 134), # sqrt(3.36e5 x 1.5e6) = 7.1e5: 119 pairs
    (EUCLIDEAN_ERROR, EST_RANSAC, 1157, 300, 3, 14, 26),     # 2.4e4: 20 pairs (hb - 1 = 4; alone: 50)
]

# one input tuple: the call's shape, the context's options under their public names, and `veto` = the "nothing to gain" policy
# sends a call that the cost model would stage to complete scoring
INPUT_FIELDS = ("family", "mode", "estimator", "P", "cap", "H", "side_by_side", "prune", "reorder", "gensplit", "singlerest", "pretest",
                "prefix", "msplit", "list_g2", "model_room_mib", "complete", "adaptive", "veto")
HEAD_FIELDS = ("wants_staged", "staged", "status")
DECISION_FIELDS = ("msplit", "genSplit", "genPlain", "reorder", "prefix", "lastStage", "big0", "modelH", "parkModels", "skipE", "skipF",
                   "zeroCounts", "zeroH")
BLOCKS = ("counts", "models", "validMask", "survA", "survB", "survN", "recF2", "permBuf", "prefInfo", "frontRec")
SCHEDULE_FIELDS = ("launches", "reorderBefore", "pretest")
LAUNCH_FIELDS = ("kind", "loop", "stage", "genOnly", "hBase", "hCount", "groups", "msplit", "validMask", "perm", "frontRec", "listIn", "listOut",
                 "single", "loopGroups")


def input_line(row_in):
    return " ".join(str(int(row_in[f])) for f in INPUT_FIELDS)


def parse_output(line, launch_fields=LAUNCH_FIELDS):
    """One printed line (or its numbers) -> {"wants_staged", "staged", "status"} and, unless the batch is refused, "decision", "bytes",
    "reorderBefore", "pretest" and the launch list."""
    v = [int(x) for x in line.split()] if isinstance(line, str) else list(line)
    out = dict(zip(HEAD_FIELDS, v[:3]))
    v = v[3:]
    if out["status"] != PS_OK:
        assert not v, line
        return out
    out["decision"] = dict(zip(DECISION_FIELDS, v))
    v = v[len(DECISION_FIELDS):]
    out["bytes"] = dict(zip(BLOCKS, v))
    v = v[len(BLOCKS):]
    n, out["reorderBefore"], out["pretest"] = v[:3]
    v = v[3:]
    assert len(v) == n * len(launch_fields), line
    out["launches"] = [dict(zip(launch_fields, v[i * len(launch_fields):(i + 1) * len(launch_fields)])) for i in range(n)]
    return out


BOOLEAN_DECISIONS = ("genSplit", "genPlain", "reorder", "big0", "parkModels", "skipE", "skipF", "zeroCounts")


def coverage(rows):
    """What a table of parsed rows has to show, name -> whether it does: every boolean decision with both values, both values of lastStage,
    fewer model slots than hypotheses, looping work-groups, the refusal, and each of the five launch shapes."""
    ok = [(r_in, r) for r_in, r in rows if r["status"] == PS_OK]
    cov = {"refusal": any(r["status"] == PS_ERR_UNSUPPORTED for _, r in rows)}
    for name in ("wants_staged", "staged"):
        cov[name] = {r[name] for _, r in rows} == {0, 1}
    cov["veto"] = any(r["wants_staged"] and not r["staged"] for _, r in rows)
    cov["pretest"] = {r["pretest"] for _, r in ok} == {0, 1}
    for name in BOOLEAN_DECISIONS:
        cov[name] = {r["decision"][name] for _, r in ok} == {0, 1}
    cov["lastStage"] = {r["decision"]["lastStage"] for _, r in ok if r["staged"]} == {1, K_STAGES}
    cov["modelH < H"] = any(r["decision"]["modelH"] < r_in["H"] for r_in, r in ok)
    cov["loopGroups > 0"] = any(l["loopGroups"] > 0 for _, r in ok for l in r["launches"])
    shapes = [[(l["kind"], l["loop"], l["genOnly"], l["msplit"]) for l in r["launches"]] for _, r in ok if r["launches"]]
    staged = [[l for l in r["launches"]] for _, r in ok if r["staged"] and r["launches"]]
    cov["plain"] = any(len(s) == 1 and s[0][0] == 0 for s in shapes)
    cov["genPlain pair"] = any(r["decision"]["genPlain"] and [l["genOnly"] for l in r["launches"]] == [1, 0] for _, r in ok)
    cov["genSplit pair"] = any(r["decision"]["genSplit"] and [l["genOnly"] for l in r["launches"][:2]] == [1, 0] and len(r["launches"]) > 2 for _, r in ok)
    cov["looping stage 1"] = any(l["kind"] == 1 and l["loop"] for s in staged for l in s)
    cov["list stages with rsplit 4"] = any(l["kind"] == 2 and l["stage"] == K_STAGES and l["msplit"] == 4 for s in staged for l in s)
    return cov
