#!/usr/bin/env python3
"""What the convergence metric costs (PtOptions.convergence): whole-batch Msamples/s with the metric off and on,
alternating, for the bench.py configuration (cornell 1080p, depth 8, fast) on the whole frame and on the tile one of eight
GPUs renders (tools/small_tiles.py geometry).  Medians with their spread over the repetitions.
usage: tools/convergence_cost.py [--reps 5] [--steps 500] [--worlds 1,8] [--once]
--once: one short render per setting and nothing timed on the host — the run to put under `rocprofv3 --kernel-trace --stats`
(k_collect is the gather with the metric off, k_collect_conv with it on) or `--pmc`."""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosc_4397_pathtracing_raytracing_project_amd import capi, parallel, scenes  # noqa: E402

W, H = 1920, 1080


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--worlds", default="1,8")
    ap.add_argument("--settings", default="0,1", help="PtOptions.convergence values to compare (1: every iteration but the first pays)")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    path = scenes.write_scene(scenes.cornell_scene_text(res=(W, H)), os.path.join(tempfile.mkdtemp(), "cornell.txt"))
    sc = capi.Scene(path, res=(W, H))
    settings = [int(v) for v in a.settings.split(",")]
    for world in (int(v) for v in a.worlds.split(",")):
        tile = parallel.striped_tile_for_rank(W, H, 0, world) if world > 1 else dict(pixel_begin=0, pixel_count=W * H)
        n = tile["pixel_count"]
        rates = {c: [] for c in settings}
        for rnd in range(1 if a.once else 2):  # off, on, off, on: a drift of the machine shows as a difference between the rounds
            for conv in settings:
                r = capi.Renderer(sc, arith="fast", convergence=conv, **tile)
                try:
                    k = r.stats().iters_per_batch
                    steps = 2 * k if a.once else max(k, a.steps // k * k)  # whole batches
                    r.render(1, 2 * k)
                    r.sync()
                    for _ in range(0 if a.once else a.reps):
                        r.clear()
                        r.sync()
                        t0 = time.perf_counter()
                        r.render(1, steps)
                        r.sync()
                        rates[conv].append(n * steps / (time.perf_counter() - t0) / 1e6)
                    if conv:
                        last = r.convergence(steps, 1)[0]
                        print(f"  (world {world}, convergence {conv}: sse of iteration {steps} = {last!r})", flush=True)
                finally:
                    r.free()
        if a.once:
            continue
        for conv in settings:
            v = sorted(rates[conv])
            print(f"world {world} tile {n} px K={k} steps={steps} convergence={conv}: median {statistics.median(v):8.1f} Msamples/s  "
                  f"min {v[0]:8.1f} max {v[-1]:8.1f}  (n={len(v)})", flush=True)
        base = statistics.median(rates[settings[0]])
        for conv in settings[1:]:
            print(f"world {world}: convergence={conv} / convergence={settings[0]} = {statistics.median(rates[conv]) / base:.4f}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
