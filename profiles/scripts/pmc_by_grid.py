#!/usr/bin/env python3
"""Every counter of one or more `rocprofv3 --pmc` passes per step and launch shape (the format of sq_counters_by_grid.json).

Each input is the counter_collection CSV of a pass of its own, no tracing beside it; passes of the same library with
different counters merge into one table:

    PUTSLAM_HIP_LIB=<library> rocprofv3 --pmc <counters> --output-format csv -d <dir> -o bench -- \
        python3 bench.py --gpus 1 --full --streams 1 --steps 20 --warmup 20 --warm-seconds 0 --repeats 1 --no-other-modes \
        --no-cpu-baseline --no-native-legs --no-streamed --no-data-legs --no-latency --no-stress

usage: pmc_by_grid.py <out.json> <pass.csv> [<pass.csv> ...]
Steps = dispatches of the once-per-step kernel ps_crosscheck_prep; a value is the mean over the launches of its shape."""
import collections
import csv
import json
import sys


def load(path, into):
    by = collections.defaultdict(lambda: collections.defaultdict(list))
    for r in csv.DictReader(open(path)):
        k = r["Kernel_Name"]
        if "psdev::" in k:
            name = k.split("psdev::")[1].split("(")[0]
            by["%s grid %s" % (name, r["Grid_Size"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
    nstep = max(len(v) for k, c in by.items() if k.startswith("ps_crosscheck_prep") for v in c.values())
    for k, c in by.items():
        e = into.setdefault(k, {})
        for n, v in c.items():
            e[n] = sum(v) / len(v)
            e["launches_per_step"] = len(v) / nstep
    return nstep


def main():
    out = {}
    steps = [load(p, out) for p in sys.argv[2:]]
    total = collections.Counter()
    for k, e in out.items():
        for n, v in e.items():
            if n != "launches_per_step":
                total[n] += v * e["launches_per_step"]
    out["whole step"] = dict(total)
    json.dump(out, open(sys.argv[1], "w"), indent=1, sort_keys=True)
    print("steps", steps)
    for k in sorted(out):
        print("%-64s %s" % (k, {n: round(v) for n, v in sorted(out[k].items()) if n != "launches_per_step"}))


if __name__ == "__main__":
    main()
