#!/usr/bin/env python3
"""What the noise estimate costs (pt_noise_fold / pt_render_until): Msamples/s of plain pt_render and of
pt_render_until with a target out of reach (so both render the same iterations), alternating, for the bench.py configuration
(cornell 1080p, depth 8, fast).  render_until folds and synchronises once per group; group_iters 0 = one batch.
usage: tools/noise_cost.py [--reps 5] [--steps 500] [--group 0] [--once]
--once: a few batches with a fold after each and nothing timed on the host — the run to put under
`rocprofv3 --kernel-trace --stats` (k_noise_fold, k_noise_reduce beside k_primary, k_paths, k_collect)."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--group", type=int, default=0)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    path = scenes.write_scene(scenes.cornell_scene_text(res=(W, H)), os.path.join(tempfile.mkdtemp(), "cornell.txt"))
    r = capi.Renderer(capi.Scene(path, res=(W, H)), arith="fast")
    n = W * H
    try:
        k = r.stats().iters_per_batch
        if a.once:
            for g in range(8):
                r.render(1 + g * k, k)
                r.noise_fold()
            print(f"K={k}: 8 batches, 8 folds; {r.noise()}", flush=True)
            return 0
        steps = max(k, a.steps // k * k)  # whole batches
        r.render(1, 2 * k)
        r.noise_fold()  # the state is allocated before anything is timed
        r.sync()
        rates = {"render": [], "render_until": []}
        for _ in range(a.reps):
            for what in rates:
                r.clear()
                r.sync()
                t0 = time.perf_counter()
                if what == "render":
                    r.render(1, steps)
                    r.sync()
                else:
                    done, db = r.render_until(1, steps, 99.0, group_iters=a.group)
                    assert done == steps
                rates[what].append(n * steps / (time.perf_counter() - t0) / 1e6)
        noise = r.noise()
        print(f"render_until: {noise['groups']} groups, {noise['iterations']} iterations, estimated PSNR {db:.3f} dB", flush=True)
        for what, v in rates.items():
            v = sorted(v)
            print(f"1080p K={k} steps={steps} group={a.group or k} {what:13s}: median {statistics.median(v):8.1f} Msamples/s  min {v[0]:8.1f} max {v[-1]:8.1f}  (n={len(v)})",
                  flush=True)
        print(f"render_until / render = {statistics.median(rates['render_until']) / statistics.median(rates['render']):.4f}", flush=True)
    finally:
        r.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
