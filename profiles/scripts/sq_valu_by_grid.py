#!/usr/bin/env python3
"""SQ_INSTS_VALU per step and launch shape of two libraries, side by side (the format of sq_counters_by_grid.json).

Each input is the counter_collection CSV of ONE pass of its own, no tracing beside it:

    PUTSLAM_HIP_LIB=<library> rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d <dir> -o bench -- \
        python3 bench.py --full --streams 1 --steps 20 --warmup 20 --warm-seconds 0 --repeats 1 --no-other-modes \
        --no-cpu-baseline --no-native-legs --no-streamed --no-data-legs --no-latency --no-stress

usage: sq_valu_by_grid.py <before.csv> <after.csv> <before.json> <after.json>
Steps = dispatches of the once-per-step kernel ps_crosscheck_prep; the last line sums the scoring launches."""
import collections
import csv
import json
import sys


def load(path):
    by = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        k = r["Kernel_Name"]
        if "psdev::" in k and r["Counter_Name"] == "SQ_INSTS_VALU":
            name = k.split("psdev::")[1].split("(")[0]
            grid = r.get("Grid_Size") or r.get("Grid_Size_X") or "?"
            by[f"{name} grid {grid}"].append(float(r["Counter_Value"]))
    nstep = max(len(v) for k, v in by.items() if k.startswith("ps_crosscheck_prep"))
    return {k: {"SQ_INSTS_VALU": sum(v) / nstep, "launches_per_step": len(v) / nstep} for k, v in by.items()}, nstep


def main():
    a, na = load(sys.argv[1])
    b, nb = load(sys.argv[2])
    print("steps", na, nb)
    ta = tb = 0.0
    for k in a:
        x, y = a[k]["SQ_INSTS_VALU"], b.get(k, {}).get("SQ_INSTS_VALU", float("nan"))
        if "ps_ransac_score_fast" in k:
            ta += x
            tb += y
        print("%-62s %14.0f %14.0f %+12.0f" % (k, x, y, y - x))
    print("scoring launches %.0f %.0f %+.0f" % (ta, tb, tb - ta))
    json.dump(a, open(sys.argv[3], "w"), indent=1)
    json.dump(b, open(sys.argv[4], "w"), indent=1)


if __name__ == "__main__":
    main()
