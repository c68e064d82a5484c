#!/usr/bin/env python3
"""What adaptive sampling by threshold (pt_render_threshold) costs and buys on the GPU; profiles/adaptive_threshold_cost.log is this
tool's output (sections 1 - 4) followed by the benchmark of the default path (section 5, bench.py runs of their own).

  tools/adaptive_threshold_cost.py [--res WxH] [--group G] [--target-spp S] [--cap F ...] [--min-pixels P ...] [--log FILE]

Cornell, exact arithmetic, no jitter, groups of G iterations.
  1. The threshold: uniform groups are folded up to S iterations, the noise planes read back, and the smallest threshold at which no
     pixel is above (pt_adaptive_select_threshold_host, bisected) becomes the run's threshold, so that uniform sampling needs about
     S iterations to meet the criterion.
  2. Uniform sampling to the criterion: groups with a fold each, planes read back and counted on the host after every group; the
     count of groups is then rendered again without the readbacks and timed (host clock around work that ends in a synchronise,
     after a warm-up of the same shape).
  3. pt_render_threshold for every cap fraction and floor: wall time (same clock), iteration numbers, samples, pixels left above.
  4. The same run round by round (pt_adaptive_round_threshold, which synchronises, so the host clock brackets a round): list length
     and time per round; and the time of a round that selects nothing, which is key + select + the 8-byte readback + the
     synchronise and nothing else.
No timing is asserted anywhere."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes  # noqa: E402


class Log:
    def __init__(self, path):
        self.f = open(path, "w") if path else None

    def __call__(self, text=""):
        print(text, flush=True)
        if self.f:
            self.f.write(text + "\n")
            self.f.flush()


def raw_planes(r):
    out = np.empty((capi.NOISE_PLANES, r.n, 4), np.float32)
    capi._check(capi.lib().pt_readback_noise(capi._f(out)))
    return out


def above(r, W, H, threshold):
    return capi.adaptive_select_threshold_host(raw_planes(r), r.readback_adaptive(), W, H, threshold, 1)[1]


def timed(work, r):
    """Seconds of the second of two runs of work() (the first warms the shape up); each ends in a synchronise."""
    for _ in range(2):
        r.clear()
        r.sync()
        t0 = time.perf_counter()
        out = work()
        r.sync()
        dt = time.perf_counter() - t0
    return dt, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", default="1920x1080")
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--target-spp", type=int, default=300, help="iterations uniform sampling should need for the criterion")
    ap.add_argument("--max-spp", type=int, default=500, help="where the search for uniform's count gives up")
    ap.add_argument("--cap", type=float, nargs="+", default=[0.25, 1.0])
    ap.add_argument("--min-pixels", type=int, nargs="+", default=[0, 64])
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    W, H = (int(v) for v in a.res.split("x"))
    n, G = W * H, a.group
    log = Log(a.log)
    path = scenes.write_scene(scenes.cornell_scene_text(), os.path.join(tempfile.mkdtemp(), "cornell.txt"))
    r = capi.Renderer(capi.Scene(path, res=(W, H)), arith="exact")
    try:
        log(f"Adaptive sampling by threshold (pt_render_threshold): cornell {W}x{H}, depth {r.scene.trace_depth}, exact, groups of {G}.")
        # ---- 1. the threshold ----
        groups = max(2, a.target_spp // G)
        for j in range(groups):
            r.render(1 + j * G, G)
            r.noise_fold()
        planes, counts = raw_planes(r), r.readback_adaptive()
        lo, hi = 0.0, 1.0
        while capi.adaptive_select_threshold_host(planes, counts, W, H, hi, 1)[1] > 0:
            hi *= 2.0
        for _ in range(40):  # the smallest threshold with nothing above, to float32's resolution
            mid = 0.5 * (lo + hi)
            lo, hi = (lo, mid) if capi.adaptive_select_threshold_host(planes, counts, W, H, mid, 1)[1] == 0 else (mid, hi)
        threshold = float(np.float32(hi))
        log(f"\n== 1. The threshold ==\nAfter {groups} uniform groups ({groups * G} spp) no pixel's estimated standard error is above {threshold:.6g}: the threshold of every run below.")
        # ---- 2. uniform sampling to the criterion ----
        log("\n== 2. Uniform sampling to the criterion (pixels above the threshold after every folded group) ==")
        r.clear()
        need = {}
        for j in range(a.max_spp // G):
            r.render(1 + j * G, G)
            r.noise_fold()
            if j >= 1:
                left = above(r, W, H, threshold)
                log(f"uniform {(j + 1) * G:5d} spp: {left:8d} pixels above")
                for floor in a.min_pixels:
                    if left <= floor and floor not in need:
                        need[floor] = j + 1
                if len(need) == len(a.min_pixels):
                    break

        def uniform(count):
            for j in range(count):
                r.render(1 + j * G, G)
                r.noise_fold()

        uniform_time = {}
        for floor, count in sorted(need.items()):
            uniform_time[floor], _ = timed(lambda: uniform(count), r)
            log(f"uniform meets the criterion (at most {floor} pixels above) after {count} groups = {count * G} spp = {count * G * n} samples: "
                f"{uniform_time[floor] * 1e3:.2f} ms, {count * G * n / uniform_time[floor] / 1e6:.0f} Msamples/s")
        for floor in a.min_pixels:
            if floor not in need:
                log(f"uniform does not meet the criterion (at most {floor} pixels above) within {a.max_spp} spp")
        # ---- 3. pt_render_threshold ----
        log("\n== 3. pt_render_threshold: wall time and samples against uniform sampling to the same criterion ==")
        for cap in a.cap:
            for floor in a.min_pixels:
                dt, (done, samples, left) = timed(lambda: r.render_threshold(1, 100 * a.max_spp, threshold, max_fraction=cap, group_iters=G, min_pixels=floor), r)
                rounds = r.noise()["groups"] - 2
                line = (f"cap {cap:4.2f}, floor {floor:3d}: {dt * 1e3:8.2f} ms, {done} iteration numbers, {rounds} rounds, {samples} samples = {samples / n:.1f} spp, "
                        f"{left} pixels left above, device bytes {r.stats().device_bytes}")
                if floor in need:
                    us, ut = need[floor] * G * n, uniform_time[floor]
                    line += f"; against uniform: samples x{samples / us:.3f}, time x{dt / ut:.3f}"
                log(line)
        # ---- 4. round by round ----
        cap = a.cap[0]
        log(f"\n== 4. Round by round (cap {cap}, floor 0; pt_adaptive_round_threshold synchronises, the host clock brackets a round) ==")
        for run in range(2):  # the first pass warms up
            r.clear()
            uniform(2)
            r.sync()
            rows, k = [], 0
            while k < 100 * a.max_spp // G:
                t0 = time.perf_counter()
                left, m = r.adaptive_round_threshold(1 + (2 + k) * G, G, threshold, cap)
                r.sync()
                rows.append((k, left, m, time.perf_counter() - t0))
                if m == 0:
                    break
                k += 1
        for k, left, m, dt in rows:
            log(f"round {k:3d}: {left:8d} above, list {m:8d}, {dt * 1e3:8.3f} ms" + (f", {G * m / dt / 1e6:8.0f} Msamples/s" if m else "  (selects nothing: key + select + readback + synchronise)"))
        empty = []
        for _ in range(20):
            t0 = time.perf_counter()
            r.adaptive_round_threshold(1, G, 1e18, cap)
            empty.append(time.perf_counter() - t0)
        total = sum(row[3] for row in rows)
        log(f"a round that selects nothing: median {np.median(empty) * 1e6:.0f} us, min {min(empty) * 1e6:.0f} us of 20; {len(rows)} selections x the median = "
            f"{len(rows) * np.median(empty) * 1e3:.2f} ms of the {total * 1e3:.2f} ms the rounds took ({len(rows) * np.median(empty) / total:.3f})")
        short = [row for row in rows if 0 < row[2] < 4096]
        if short:
            log(f"{len(short)} of the {len(rows) - 1} rendering rounds hold fewer than 4096 pixels: {sum(row[3] for row in short) * 1e3:.2f} ms for "
                f"{sum(G * row[2] for row in short)} samples ({sum(row[2] for row in short) / max(1, sum(row[2] for row in rows)):.4f} of the rounds' samples)")
    finally:
        r.free()


if __name__ == "__main__":
    main()
