#!/usr/bin/env python3
"""What adaptive sampling costs and buys on the GPU (profiles/adaptive_cost.log is this tool's output).

  tools/adaptive_cost.py round [--res WxH] [--group G] [--fraction F] [--rounds R]
      The workload for `rocprofv3 --kernel-trace --stats -- python tools/adaptive_cost.py round` (a run of its own, no counters):
      two uniform groups of G iterations with their folds, then R rounds.  Prints the samples of each part, so that the kernel
      times of the trace can be turned into time per sample.
  tools/adaptive_cost.py stats FILE_kernel_stats.csv --group G --fraction F --rounds R [--res WxH]
      Adds the trace's kernel times up by part: key + select + merge, the worker's path-tracing kernels per sample against the
      whole-frame renderer's per sample.  The worker's launches are told from the renderer's by their order in the run, so this
      reads the per-call trace (FILE_kernel_trace.csv) next to the stats file.
  tools/adaptive_cost.py headline [--res WxH] [--group G] [--fraction F] [--truth-spp N]
      Wall time (host clock around work that ends in a synchronise, after a warm-up of the same shape) and samples of uniform
      rendering and of adaptive rendering at several budgets, each with its ACTUAL PSNR against a truth-spp render of the same
      build, and for every adaptive point the uniform samples and time that reach the same actual PSNR (interpolated in log spp).
"""
import argparse
import csv
import math
import os
import re
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes  # noqa: E402

SELECT = ("k_adaptive_key", "k_adaptive_hist", "k_adaptive_pick", "k_adaptive_count", "k_adaptive_scan", "k_adaptive_scatter")
MERGE = ("k_adaptive_merge", "k_adaptive_partial", "k_noise_reduce")
TRACE = ("k_primary", "k_paths", "k_collect")


def renderer(res, **kw):
    td = tempfile.mkdtemp()
    path = scenes.write_scene(scenes.cornell_scene_text(), os.path.join(td, "cornell.txt"))
    return capi.Renderer(capi.Scene(path, res=res), **kw)


def run_round(a):
    n = a.res[0] * a.res[1]
    m = int(min(n, max(1, math.ceil(a.fraction * n))))
    r = renderer(a.res)
    try:
        for j in range(2):
            r.render(1 + j * a.group, a.group)
            r.noise_fold()
        for k in range(a.rounds):
            r.adaptive_round(1 + (2 + k) * a.group, a.group, a.fraction)
        r.sync()
        st = r.stats()
        print(f"round: {a.res[0]}x{a.res[1]}, G = {a.group}, fraction {a.fraction}: uniform samples {2 * a.group * n}, "
              f"worker samples {a.rounds * a.group * m} in {a.rounds} round(s) over {m} pixels, PtStats.samples {st.samples}, "
              f"device bytes {st.device_bytes}, whole-frame iterations per batch {st.iters_per_batch}")
    finally:
        r.free()


def run_stats(a):
    trace = a.csv.replace("kernel_stats", "kernel_trace")
    rows = list(csv.DictReader(open(trace)))
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    name = lambda x: x["Kernel_Name"]
    dur = lambda x: (int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) * 1e-3  # us
    # the first round starts at the first k_adaptive_init_counts / k_adaptive_key launch: path-tracing kernels before it are the
    # whole-frame renderer's, after it the worker's.  The renderer's timing batches at init (choose_traversal) do not exist for cornell.
    first = next(i for i, x in enumerate(rows) if "k_adaptive" in name(x))
    n = a.res[0] * a.res[1]
    m = int(min(n, max(1, math.ceil(a.fraction * n))))
    part = lambda rs, keys: {k: sum(dur(x) for x in rs if re.search(r"\b" + k + r"\b", name(x))) for k in keys}
    frame, worker = part(rows[:first], TRACE), part(rows[first:], TRACE)
    sel, mer = part(rows[first:], SELECT), part(rows[first:], MERGE)
    us, ws = 2 * a.group * n, a.rounds * a.group * m
    print(f"per round: key + select {sum(sel.values()) / a.rounds:.1f} us {({k: round(v / a.rounds, 1) for k, v in sel.items()})}")
    print(f"per round: merge + SSE {sum(mer.values()) / a.rounds:.1f} us {({k: round(v / a.rounds, 1) for k, v in mer.items()})}")
    print(f"per round: the worker's k_primary + k_paths + k_collect {sum(worker.values()) / a.rounds:.1f} us")
    for k in TRACE:
        f, w = frame[k] * 1e3 / us, worker[k] * 1e3 / ws
        print(f"  {k:10s} whole frame {f:.4f} ns/sample, worker {w:.4f} ns/sample ({w / f:.2f}x)" if f > 0 else f"  {k}: not in the trace")
    f, w = sum(frame.values()) * 1e3 / us, sum(worker.values()) * 1e3 / ws
    print(f"  all three  whole frame {f:.4f} ns/sample ({1e3 / f:.0f} Msamples/s), worker {w:.4f} ns/sample ({1e3 / w:.0f} Msamples/s): the worker's rate is {f / w:.2f} of the whole frame's")
    print(f"  selection + merge are {(sum(sel.values()) + sum(mer.values())) / (sum(sel.values()) + sum(mer.values()) + sum(worker.values())):.3f} of a round's kernel time")


def psnr(img, truth, n):
    return capi.psnr_from_sse(float(((img.astype(np.float64) - truth) ** 2).sum()), n)


def run_headline(a):
    n = a.res[0] * a.res[1]
    r = renderer(a.res)
    try:
        r.render(1000001, a.truth_spp)
        truth = r.readback().astype(np.float64) / a.truth_spp
        uniform = []
        for spp in (2 * a.group, 3 * a.group, 4 * a.group, 6 * a.group, 8 * a.group, 12 * a.group, 16 * a.group):
            for timed in (False, True):  # the first pass warms the shape up
                r.clear()
                t0 = time.perf_counter()
                done, est = r.render_until(1, spp, 200.0, group_iters=a.group)  # groups and folds, as a user who wants an estimate renders
                r.sync()
                dt = time.perf_counter() - t0
            uniform.append((spp, dt, psnr(r.readback() / np.float32(spp), truth, n), est))
            print(f"uniform  {spp:4d} spp: {dt * 1e3:8.2f} ms, {spp * n / dt / 1e6:8.0f} Msamples/s, actual PSNR {uniform[-1][2]:.2f} dB, estimated {est:.2f} dB")
        for worth in (3, 4, 6, 8):  # iterations' worth of samples, in units of G
            rounds = int(round((worth - 2) * a.group / (a.group * a.fraction)))
            iters = (2 + rounds) * a.group
            for timed in (False, True):
                r.clear()
                t0 = time.perf_counter()
                done, samples, est = r.render_adaptive(1, iters, 200.0, a.fraction, group_iters=a.group)
                r.sync()
                dt = time.perf_counter() - t0
            p = psnr(r.resolve(), truth, n)
            # the uniform spp with the same actual PSNR: linear in log2(spp) between the measured points
            xs, ys, ts = [math.log2(u[0]) for u in uniform], [u[2] for u in uniform], [u[1] for u in uniform]
            eq_spp = 2.0 ** float(np.interp(p, ys, xs))
            eq_ms = float(np.interp(math.log2(eq_spp), xs, ts)) * 1e3
            print(f"adaptive {samples / n:6.1f} spp ({rounds} rounds, {done} iteration numbers): {dt * 1e3:8.2f} ms, {samples / dt / 1e6:8.0f} Msamples/s, actual PSNR {p:.2f} dB, "
                  f"estimated {est:.2f} dB; uniform reaches {p:.2f} dB at {eq_spp:.1f} spp in {eq_ms:.2f} ms: samples x{samples / n / eq_spp:.2f}, time x{dt * 1e3 / eq_ms:.2f}")
    finally:
        r.free()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["round", "stats", "headline"])
    ap.add_argument("csv", nargs="?")
    ap.add_argument("--res", default="1920x1080")
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--fraction", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--truth-spp", type=int, default=4096)
    a = ap.parse_args()
    a.res = tuple(int(v) for v in a.res.split("x"))
    {"round": run_round, "stats": run_stats, "headline": run_headline}[a.mode](a)


if __name__ == "__main__":
    main()
