#!/usr/bin/env python3
"""What the reprojected history costs in a group (pt_group_history_*); profiles/group_history_cost.log is this
tool's output.

  tools/group_history_cost.py [--reps 21] [--log FILE]

Cornell and the 10,170-primitive stress scene at 1920 x 1080, fast arithmetic.  A group of two contexts on ONE device (devices [0, 0],
the COPY transport) and one context of the whole frame, in the same process, make the same calls: a view of 1 iteration, its first
hits, a capture with moments, one orbit step of 2 pi / 120, the next view and its first hits.  Then each step of a view — lookup, round,
resolve, filter, capture — is timed on its own, per repetition on the group and on the context in turn: host wall clock around the call
and the synchronise that ends it (the group's call spans the streams of its contexts, so HIP events on one stream do not bracket it).
The first repetition (allocations, code objects) is dropped; medians are printed with the bytes the group's call assembles on the root.

The same kernels run at the same size on the same device, so group minus context is the exchange and the placement of the rows: the
group form's overhead on one GPU.  It is not scaling, and on more than one GPU this has not run.  No timing is asserted anywhere."""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes  # noqa: E402

W, H, G = 1920, 1080, 1
N = W * H
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--log", default=os.devnull)
args = ap.parse_args()
out = open(args.log, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


L = capi.lib()
MOM = capi.HISTORY_MOMENTS
F = capi.FEATURE_PLANES
one = C.c_float(1.0)
hopt, ropt = capi.history_options(), capi.history_round_options(0.75, 0.25)
rgb = np.empty((N, 3), np.float32)
fresh, m = C.c_int32(-1), C.c_int32(-1)


class Single:
    """One context of the whole frame behind the names the group's calls have."""
    name = "context"

    def __init__(self, scene, opt):
        self.h = C.c_void_p()
        capi._check(L.pt_ctx_create(C.byref(scene.desc), C.byref(opt), C.byref(self.h)))

    def sync(self): return L.pt_ctx_sync(self.h)
    def render(self, first, n): return L.pt_ctx_render(self.h, first, n)
    def features(self): return L.pt_ctx_render_features(self.h, 1, 1)
    def move(self, cam): return L.pt_ctx_set_camera(self.h, C.byref(cam))
    def lookup(self): return L.pt_ctx_history_reproject_ex(self.h, C.byref(hopt), MOM)
    def round(self, first): return L.pt_ctx_history_round(self.h, first, G, C.byref(ropt), C.byref(fresh), C.byref(m))
    def resolve(self): return L.pt_ctx_history_resolve(self.h, one, capi._f(rgb))
    def filter(self): return L.pt_ctx_history_denoise_ex(self.h, one, None, MOM, capi._f(rgb))
    def capture(self): return L.pt_ctx_history_capture_ex(self.h, one, MOM)
    def free(self): L.pt_ctx_destroy(self.h)


class Pair:
    """A group of two contexts on device 0."""
    name = "group"

    def __init__(self, scene, opt):
        self.h = C.c_void_p()
        dev = np.zeros(2, np.int32)
        capi._check(L.pt_group_create(C.byref(scene.desc), C.byref(opt), capi._i(dev), 2, C.byref(self.h)))

    def sync(self): return L.pt_group_sync(self.h)
    def render(self, first, n): return L.pt_group_render(self.h, first, n)
    def features(self): return L.pt_group_render_features(self.h, 1, 1)
    def move(self, cam): return L.pt_group_set_camera(self.h, C.byref(cam))
    def lookup(self): return L.pt_group_history_reproject_ex(self.h, C.byref(hopt), MOM)
    def round(self, first): return L.pt_group_history_round(self.h, first, G, C.byref(ropt), C.byref(fresh), C.byref(m))
    def resolve(self): return L.pt_group_history_resolve(self.h, one, capi._f(rgb))
    def filter(self): return L.pt_group_history_denoise_ex(self.h, one, None, MOM, capi._f(rgb))
    def capture(self): return L.pt_group_history_capture_ex(self.h, one, MOM)
    def free(self): L.pt_group_destroy(self.h)


def timed(x, call):
    """Median of the wall-clock milliseconds of call(rep) and the synchronise that ends it; the first repetition dropped."""
    t = []
    for rep in range(args.reps):
        capi._check(x.sync())
        t0 = time.perf_counter()
        capi._check(call(rep))
        capi._check(x.sync())
        if rep:
            t.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(t)


say(f"# pt_group_history_* on devices [0, 0] beside pt_ctx_history_* on one context of the whole frame, same process, MI355X, {W} x {H}, fast arithmetic")
say(f"# medians of {args.reps - 1} repetitions, host wall clock around each call and the synchronise that ends it, in ms; the resolve and the filter return {12 * N / 1e6:.1f} MB to the host in both forms")
say("# gathered: the bytes per frame pixel the group's call assembles on the root (S 12, the feature planes 16 each, E 4), each through one exchange of")
say("# context 1's rows (half the frame) and one placement of every row; group - context is that exchange and placement: the group form's overhead")
say("# on ONE GPU.  It is not scaling, and on more than one GPU (the RCCL transport, xGMI) this has not run.")
tmp = tempfile.mkdtemp()
STEPS = (("lookup", 16 * F), ("round", 16 * F), ("resolve", 12 + 4), ("filter", 12 + 16 * F + 4), ("capture", 12 + 16 * F + 4))
for name, text in (("cornell (7 primitives)", scenes.cornell_scene_text(res=(W, H))), ("stress 22x22x21 (10170 primitives)", scenes.stress_scene_text())):
    path = scenes.write_scene(text, os.path.join(tmp, "s.txt"))
    scene = capi.Scene(path, res=(W, H))
    opt = capi.make_options(arith="fast")
    pair, single = Pair(scene, opt), Single(scene, opt)
    try:
        cam = scene.orbit(np.float32(2 * np.pi / 120), 0.0, 0.0)
        t = {}
        for x in (pair, single):
            capi._check(x.render(1, 1) or x.features() or x.capture() or x.move(cam) or x.render(2, 1) or x.features())
            t[x.name, "render"] = timed(x, lambda rep: x.render(100 + rep, 1))
            t[x.name, "features"] = timed(x, lambda rep: x.features())
            t[x.name, "lookup"] = timed(x, lambda rep: x.lookup())
            t[x.name, "round"] = timed(x, lambda rep: x.round(1000 + rep * G))
            t[x.name, "selected"] = (fresh.value, m.value)
            t[x.name, "resolve"] = timed(x, lambda rep: x.resolve())
            t[x.name, "filter"] = timed(x, lambda rep: x.filter())
            t[x.name, "capture"] = timed(x, lambda rep: x.capture())
        assert t["group", "selected"] == t["context", "selected"], t
        say(f"\n## {name}: the round selects {t['group', 'selected'][1]} of {t['group', 'selected'][0]} fresh pixels, {G} iteration(s); group buffers "
            f"{L.pt_group_device_bytes(pair.h) / 2**20:.1f} MB on the root")
        say(f"{'step':10s} {'group':>10s} {'context':>10s} {'group - context':>16s} {'gathered B/pixel':>17s} {'MB':>8s}")
        for step in ("render", "features"):
            say(f"{step:10s} {t['group', step]:10.3f} {t['context', step]:10.3f} {t['group', step] - t['context', step]:16.3f} {'-':>17s} {'-':>8s}")
        over = 0.0
        for step, b in STEPS:
            d = t["group", step] - t["context", step]
            over += d
            say(f"{step:10s} {t['group', step]:10.3f} {t['context', step]:10.3f} {d:16.3f} {b:17d} {b * N / 1e6:8.1f}")
        view = sum(t["group", s] for s in ("render", "features") + tuple(s for s, _ in STEPS))
        alone = sum(t["context", s] for s in ("render", "features") + tuple(s for s, _ in STEPS))
        say(f"a view of one iteration (render, features and the five steps): group {view:.3f} ms, context {alone:.3f} ms; the five steps' gathers "
            f"take {over:.3f} ms = {100 * over / view:.1f} % of the group's view, of which the feature planes are assembled four times "
            f"({4 * 16 * F * N / 1e6:.0f} of {sum(b for _, b in STEPS) * N / 1e6:.0f} MB)")
    finally:
        pair.free()
        single.free()
out.close()
