#!/usr/bin/env python3
"""What the group form of adaptive sampling by threshold (pt_group_render_threshold) costs against a single context;
profiles/group_threshold_cost.log is this tool's output.

  tools/group_threshold_cost.py [--res WxH] [--group G] [--threshold T] [--cap F] [--devices 0,0] [--max-iters N] [--log FILE]

Cornell, exact arithmetic, no jitter, groups of G iterations: the configuration of tools/adaptive_threshold_cost.py, whose threshold
(the standard error uniform sampling reaches after 300 spp at 1920x1080) is the default here.
  1. One renderer: pt_render_threshold, wall time; then round by round (pt_adaptive_round_threshold synchronises, so the host clock
     brackets a round), and the time of a round that selects nothing: key + select + the 8-byte readback + the synchronise.
  2. A group over --devices (the default {0, 0}: two contexts on ONE GPU, which measures what the group form adds, not scaling):
     the same two runs.  A group's round that selects nothing is pack + exchange + key + select + partition + the (8 + 4n)-byte
     readback + the synchronise; what a rendering round takes beyond that is distribute + render + merge on every context.
  3. The two resolved images, compared bit for bit.
Host clock around work that ends in a synchronise, the second of two runs of the same shape.  No timing is asserted anywhere."""
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


class GroupRun:
    """A group behind the names the measurement uses of a Renderer."""

    def __init__(self, g):
        self.g = g
        self.n_ctx = capi.lib().pt_group_size(g._h)
        for name in ("render", "noise_fold", "noise", "resolve", "render_threshold", "adaptive_round_threshold"):
            setattr(self, name, getattr(g, name))

    def sync(self):
        capi._check(capi.lib().pt_group_sync(self.g._h))

    def clear(self):
        for i in range(self.n_ctx):
            capi._check(capi.lib().pt_ctx_clear(self.g.context(i)))

    def device_bytes(self):
        return sum(self.g.stats(i).device_bytes for i in range(self.n_ctx))


class SingleRun:
    def __init__(self, r):
        self.r = r
        for name in ("render", "noise_fold", "noise", "resolve", "render_threshold", "adaptive_round_threshold", "sync", "clear"):
            setattr(self, name, getattr(r, name))

    def device_bytes(self):
        return self.r.stats().device_bytes


def measure(log, x, name, n, G, threshold, cap, max_iters):
    for _ in range(2):  # the first run warms the shape up
        x.clear()
        x.sync()
        t0 = time.perf_counter()
        done, samples, left = x.render_threshold(1, max_iters, threshold, max_fraction=cap, group_iters=G)
        x.sync()
        driver = time.perf_counter() - t0
    rounds = x.noise()["groups"] - 2
    image = x.resolve()
    log(f"{name}: driver {driver * 1e3:8.2f} ms, {done} iteration numbers, {rounds} rounds, {samples} samples = {samples / n:.1f} spp, {left} pixels left above, "
        f"device bytes of the contexts {x.device_bytes()}")
    for _ in range(2):
        x.clear()
        t0 = time.perf_counter()
        for j in range(2):
            x.render(1 + j * G, G)
            x.noise_fold()
        x.sync()
        uniform = time.perf_counter() - t0
        rows, k = [], 0
        while k < max_iters // G:
            t0 = time.perf_counter()
            left, m = x.adaptive_round_threshold(1 + (2 + k) * G, G, threshold, cap)
            x.sync()
            rows.append((k, left, m, time.perf_counter() - t0))
            if m == 0:
                break
            k += 1
    empty = []
    for _ in range(20):
        t0 = time.perf_counter()
        x.adaptive_round_threshold(1, G, 1e18, cap)
        empty.append(time.perf_counter() - t0)
    select = float(np.median(empty))
    log(f"{name}: the two uniform groups with their folds {uniform * 1e3:.2f} ms; a round that selects nothing: median {select * 1e6:.0f} us, min {min(empty) * 1e6:.0f} us of 20")
    for k, left, m, dt in rows:
        log(f"{name}: round {k:3d}: {left:8d} above, list {m:8d}, {dt * 1e3:8.3f} ms" +
            (f" = {select * 1e3:.3f} selection + {(dt - select) * 1e3:8.3f} render and merge" if m else "  (selects nothing)"))
    total = sum(row[3] for row in rows)
    log(f"{name}: {len(rows)} rounds {total * 1e3:.2f} ms, of which {len(rows)} selections x the median = {len(rows) * select * 1e3:.2f} ms ({len(rows) * select / total:.3f})")
    return driver, total, select, image


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", default="1920x1080")
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--threshold", type=float, default=0.0842489, help="profiles/adaptive_threshold_cost.log: uniform sampling's after 300 spp")
    ap.add_argument("--cap", type=float, default=0.25)
    ap.add_argument("--devices", default="0,0")
    ap.add_argument("--max-iters", type=int, default=2000)
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    W, H = (int(v) for v in a.res.split("x"))
    devices = [int(v) for v in a.devices.split(",")]
    n, G = W * H, a.group
    log = Log(a.log)
    path = scenes.write_scene(scenes.cornell_scene_text(), os.path.join(tempfile.mkdtemp(), "cornell.txt"))
    scene = capi.Scene(path, res=(W, H))
    log(f"Adaptive sampling by threshold, one context against a group over devices {devices}: cornell {W}x{H}, depth {scene.trace_depth}, exact, groups of {G}, "
        f"threshold {a.threshold:.6g}, cap {a.cap}.")
    log("\n== 1. One renderer ==")
    r = capi.Renderer(scene, arith="exact")
    try:
        single = measure(log, SingleRun(r), "single", n, G, a.threshold, a.cap, a.max_iters)
    finally:
        r.free()
    log(f"\n== 2. A group of {len(devices)} contexts ==")
    g = capi.Group(scene, devices, arith="exact")
    try:
        log(f"transport {g.transport}")
        group = measure(log, GroupRun(g), "group ", n, G, a.threshold, a.cap, a.max_iters)
    finally:
        g.free()
    log("\n== 3. Group against single ==")
    same = np.array_equal(single[3].view(np.uint32), group[3].view(np.uint32))
    log(f"resolved images equal bit for bit: {same}")
    log(f"driver: group {group[0] * 1e3:.2f} ms / single {single[0] * 1e3:.2f} ms = x{group[0] / single[0]:.3f}; the rounds one by one: "
        f"{group[1] * 1e3:.2f} / {single[1] * 1e3:.2f} ms = x{group[1] / single[1]:.3f}; a selection: {group[2] * 1e6:.0f} / {single[2] * 1e6:.0f} us = x{group[2] / single[2]:.2f}")
    log(f"per frame pixel a group's selection moves 8 bytes to the root ({8 * n / 1e6:.1f} MB here), a single context's none")


if __name__ == "__main__":
    main()
