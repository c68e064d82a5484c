#!/usr/bin/env python3
"""Per-kernel counter table from `rocprofv3 --pmc` runs of bench.py, one output directory per run (counters only, no tracing):
for every directory DIR/NAME* with a *counter_collection.csv, the mean / min / max over the last three dispatches of k_primary,
k_paths, k_count_stats, k_collect and k_collect_stream (a dispatch's value = the sum over the counter's instances), and the sum over these
kernels per batch.  FETCH_SIZE / WRITE_SIZE are printed on the profiler's scale (KiB; the project's byte convention is
2 x FETCH_SIZE + WRITE_SIZE, tools/pmc_traffic.py).  The tables of profiles/retire_once.log.
usage: tools/pmc_kernels.py DIR [NAME-PREFIX]"""
import collections
import csv
import glob
import os
import sys

KERNELS = ("k_primary", "k_paths", "k_count_stats", "k_collect", "k_collect_stream")


def table(path):
    per = collections.defaultdict(lambda: collections.defaultdict(float))
    for r in csv.DictReader(open(path)):
        hit = [k for k in KERNELS if "ptk::" in r["Kernel_Name"] and k + "(" in r["Kernel_Name"].replace("<", "(")]
        if hit:
            per[(hit[0], r["Counter_Name"])][int(r["Dispatch_Id"])] += float(r["Counter_Value"])
    total = collections.defaultdict(float)
    for (k, c), v in sorted(per.items(), key=lambda kv: (KERNELS.index(kv[0][0]), kv[0][1])):
        vals = [v[i] for i in sorted(v)[-3:]]
        mean = sum(vals) / len(vals)
        print(f"  {k:14s} {c:14s} dispatches {len(v):3d}  mean of the last {len(vals)} {mean:16.1f} min {min(vals):16.1f} max {max(vals):16.1f}")
        total[c] += mean
    for c, t in total.items():
        print(f"  all kernels    {c:14s} per batch {t:16.1f}")


def main():
    root, prefix = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "pmc_"
    for d in sorted(glob.glob(os.path.join(root, prefix + "*"))):
        for f in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)):
            print("==", os.path.basename(d))
            table(f)


if __name__ == "__main__":
    main()
