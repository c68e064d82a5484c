#!/usr/bin/env python3
"""What the three forms of the à-trous filter cost (pt_denoise / pt_denoise_guided / pt_denoise_adaptive) for the
bench.py configuration (cornell 1080p, depth 8, fast): four groups of one batch with a fold after each, a feature pass, then the three
filters alternating at their defaults (the adaptive form in the uniform state: the folds' counters for every pixel).
usage: tools/denoise_cost.py [--reps 10] [--once]
--once: three calls of each and nothing timed on the host — the run to put under `rocprofv3 --kernel-trace --stats`: all eight kernels
(k_denoise_level<true> beside k_denoise_level<false>, the two k_denoise_var_prefilter<..>, the three k_denoise_prepare<..>,
k_denoise_finish).  Without it: host time per call, readback of the 25 MB result included."""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes  # noqa: E402

W, H = 1920, 1080


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    path = scenes.write_scene(scenes.cornell_scene_text(res=(W, H)), os.path.join(tempfile.mkdtemp(), "cornell.txt"))
    r = capi.Renderer(capi.Scene(path, res=(W, H)), arith="fast", aa_jitter=True)
    try:
        k = r.stats().iters_per_batch
        for g in range(4):
            r.render(1 + g * k, k)
            r.noise_fold()
        r.render_features(1, 4 * k)
        calls = {"denoise": lambda: r.denoise(4 * k), "denoise_guided": lambda: r.denoise_guided(), "denoise_adaptive": lambda: r.denoise_adaptive()}
        times = {what: [] for what in calls}
        for _ in range(3 if a.once else a.reps + 1):
            for what, call in calls.items():
                t0 = time.perf_counter()
                call()
                times[what].append((time.perf_counter() - t0) * 1e3)
        print(f"K={k}: 4 groups, {r.noise()}", flush=True)
        if not a.once:
            for what, v in times.items():
                v = sorted(v[1:])  # the first call allocates
                print(f"1080p 5 levels {what:16s}: median {statistics.median(v):7.3f} ms  min {v[0]:7.3f} max {v[-1]:7.3f}  (n={len(v)}, with the readback)", flush=True)
    finally:
        r.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
