"""Recipe of tests/golden/score_plan_parent.json: what the scoring step's plan decided BEFORE it moved into the pure header
putslam_amd/csrc/ps_score_plan.h -- prepare_score and score_schedule of putslam_amd/csrc/ps_capi.hip at commit 6fa444a -- for a
deterministic draw of input tuples.  tests/test_score_plan_host.py holds the header to every row.

The recorder is not kept in the tree.  It is those two functions' bodies transcribed into a plain C++ program: a stub context that
holds the options and one Buf per arena block, a PS_ENSURE that records the size asked for, a k3 that records the launch (its kind, its
StageArgs with each pointer named by the block it points to, groups, msplit) and the place of the ps_stage_reorder launch.  The "nothing
to gain" policy (lines 364-418 there) needs mapped memory; its outcome is the input `veto`.  The program reads one tuple per line
(tests/score_plan_rows.py: INPUT_FIELDS) and prints head, decision, block sizes and launches as test_score_plan.cpp's `plan` mode does,
with four more numbers per launch (listStride, margin, gran, c2div) that the shell in ps_capi.hip fills in by a fixed rule, checked here.

    python tests/golden/make_score_plan_parent.py <recorder executable>

Rows are redrawn (next seed) until the table meets tests/score_plan_rows.py: coverage.  No tuple of the drawn values reaches the
refusal (pairs x hypotheses x matches > 2e14; the largest is 499 x 850 000 x 4000 = 1.7e12), so rows at the bound follow the draw:
58 823 and 58 824 pairs under USAC's cap at 4000 keypoints, either side of 2e14, batched or not, staged or not."""
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import score_plan_rows as R  # noqa: E402

ROWS = 240
MODES = {R.VALUE: (0, 1, 2, 3, 4), R.EUCLID: (R.EUCLIDEAN_ERROR, R.ADAPTIVE_ERROR), R.REPROJ: (R.REPROJECTION_ERROR, R.EUCLIDEAN_AND_REPROJECTION_ERROR)}
DRAW = {"estimator": (R.EST_RANSAC, R.EST_USAC, R.EST_FIXED), "P": (1, 2, 16, 17, 48, 210, 499), "cap": (64, 500, 2000, 4000),
        "H": (256, 257, 1024, 4096, 16384, 100000, 850000), "side_by_side": (0, 2, 3), "prune": (0, 1, 2), "reorder": (0, 1, 2),
        "gensplit": (0, 1), "singlerest": (0, 1), "pretest": (0, 1), "prefix": (0, 64), "msplit": (0, 1, 8), "list_g2": (0, 3),
        "model_room_mib": (0, 1), "complete": (0, 1), "adaptive": (0, 1), "veto": (0, 0, 0, 1)}


def draw(seed):
    rng = random.Random(seed)
    rows = []
    for _ in range(ROWS):
        r = {"family": rng.choice((R.VALUE, R.EUCLID, R.REPROJ))}
        r["mode"] = rng.choice(MODES[r["family"]])
        for name, values in DRAW.items():
            r[name] = rng.choice(values)
        rows.append(r)
    for P in (58823, 58824):          # P x 850 000 x 4000 = 1.99998e14 / 2.000016e14
        for adaptive, prune, veto in ((1, 0, 0), (0, 0, 0), (1, 2, 0), (1, 2, 1)):
            r = dict(rows[0], family=R.REPROJ, mode=R.REPROJECTION_ERROR, estimator=R.EST_USAC, P=P, cap=4000, H=850000, prune=prune,
                     complete=0, adaptive=adaptive, veto=veto)
            rows.append(r)
    return rows


def main(recorder):
    extra = ("listStride", "margin", "gran", "c2div")
    for seed in range(100):
        rows_in = draw(seed)
        text = subprocess.run([recorder], input="".join(R.input_line(r) + "\n" for r in rows_in), stdout=subprocess.PIPE, text=True, check=True).stdout
        lines = text.splitlines()
        assert len(lines) == len(rows_in)
        rows = [(r_in, R.parse_output(line, R.LAUNCH_FIELDS + extra)) for r_in, line in zip(rows_in, lines)]
        cov = R.coverage(rows)
        if all(cov.values()):
            break
        print("seed", seed, "misses", [k for k, v in cov.items() if not v])
    else:
        raise SystemExit("no seed meets the coverage condition")
    out = []
    for r_in, r in rows:
        for l in r.get("launches", ()):  # the shell's rule for what the schedule does not carry
            staged = r["staged"]
            assert [l.pop(k) for k in extra] == ([r["decision"]["modelH"], 16, 64, 16] if staged else [0, 0, 0, 0]), (r_in, l)
        flat = [r[f] for f in R.HEAD_FIELDS]
        if r["status"] == R.PS_OK:
            flat += [r["decision"][f] for f in R.DECISION_FIELDS] + [r["bytes"][b] for b in R.BLOCKS]
            flat += [len(r["launches"]), r["reorderBefore"], r["pretest"]] + [l[f] for l in r["launches"] for f in R.LAUNCH_FIELDS]
        out.append({"in": [r_in[f] for f in R.INPUT_FIELDS], "out": flat})
    doc = {"commit": "6fa444a", "seed": seed, "input_fields": R.INPUT_FIELDS, "head_fields": R.HEAD_FIELDS, "decision_fields": R.DECISION_FIELDS,
           "blocks": R.BLOCKS, "schedule_fields": R.SCHEDULE_FIELDS, "launch_fields": R.LAUNCH_FIELDS}
    with open(os.path.join(HERE, "score_plan_parent.json"), "w") as f:
        f.write(json.dumps(doc)[:-1] + ', "rows": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in out) + "\n]}\n")
    print("seed", seed, "rows", len(out))


if __name__ == "__main__":
    main(sys.argv[1])
