#!/usr/bin/env python3
"""What the history probes cost (pt_history_probe_keep / _check); profiles/history_probe_cost.log is this tool's
output, beside tools/history_round_cost.py's for the steps the parent revision has too.

  tools/history_probe_cost.py [--reps 21] [--log FILE]

Cornell and the 10,170-primitive stress scene at 1920 x 1080, fast arithmetic, one context, 230,400 probes (640 x 360, phase 0).  Per
scene two passes, with k = 1 and k = 2 iterations per view: a view is rendered, its probes kept, the view captured (with moments); one
object moves by 0.5 (pt_set_geoms); the next view is rendered and looked up with PT_HISTORY_MOTION | PT_HISTORY_MOMENTS.  Then, per
repetition between HIP events on the context's stream:
  pt_history_reproject_ex   the lookup again: a new C, which a check may be applied to
  pt_history_probe_check    the list, the worker's replay of k iterations of the probes' pixels, the gradient, the apply, the 8-byte
                            readback (its one synchronise lies inside the events)
  pt_render, 1 iteration    the whole frame, for scale
and pt_history_probe_keep on its own.  The public call is one, so the check's parts are taken by difference:
  one replayed iteration    check (k = 2) - check (k = 1).  The worker traces depth 0 once per round, so this is an iteration without
                            its camera rays: the first iteration of a replay costs that much more
  list + gradient + apply   check (k = 1) - one replayed iteration: an upper bound, it holds the first iteration's camera rays too
The first repetition (allocations, code objects) is dropped.  No timing is asserted anywhere."""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--log", default=os.devnull)
args = ap.parse_args()
out = open(args.log, "a")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


import numpy as np  # noqa: E402

from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes  # noqa: E402

W, H = 1920, 1080
hip = C.CDLL("libamdhip64.so")
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
hip.hipEventDestroy.argtypes = [C.c_void_p]


def hip_ok(rc):
    if rc != 0:
        raise RuntimeError(f"HIP error {rc}")


def events(n):
    ev = [C.c_void_p() for _ in range(n)]
    for e in ev:
        hip_ok(hip.hipEventCreate(C.byref(e)))
    return ev


def elapsed(a, b):
    ms = C.c_float(0)
    hip_ok(hip.hipEventElapsedTime(C.byref(ms), a, b))
    return float(ms.value)


L = capi.lib()
L.pt_ctx_stream.argtypes = [C.c_void_p]
L.pt_ctx_stream.restype = C.c_void_p
MOM, MOTION = capi.HISTORY_MOMENTS, capi.HISTORY_MOTION


def line(what, v):
    v = sorted(v)
    med = statistics.median(v)
    say(f"{what:34s} median {med:9.4f} ms  min {v[0]:9.4f}  max {v[-1]:9.4f}  (n={len(v)})")
    return med


say(f"\n# the history probes; MI355X, {W} x {H}, fast arithmetic, {args.reps} repetitions, the first dropped; {(W // 3) * (H // 3)} probes (phase 0)")
tmp = tempfile.mkdtemp()
for name, text, geom in (("cornell (7 primitives)", scenes.cornell_scene_text(res=(W, H)), 6), ("stress 22x22x21 (10170 primitives)", scenes.stress_scene_text(), 8)):
    path = scenes.write_scene(text, os.path.join(tmp, "s.txt"))
    scene = capi.Scene(path, res=(W, H))
    opt = capi.make_options(arith="fast")
    ctx = C.c_void_p()
    capi._check(L.pt_ctx_create(C.byref(scene.desc), C.byref(opt), C.byref(ctx)))
    try:
        stream = L.pt_ctx_stream(ctx)
        hopt, popt = capi.history_options(), capi.history_probe_options()
        probes, changed, skipped = C.c_int32(0), C.c_int32(0), C.c_int32(0)

        def timed(calls, wall=None):
            """calls: (name, function) run back to back per repetition between HIP events; the first repetition is dropped."""
            ev = events(len(calls) + 1)
            t = {k: [] for k, _ in calls}
            for rep in range(args.reps):
                host = []
                for k, (_, fn) in enumerate(calls):
                    hip_ok(hip.hipEventRecord(ev[k], stream))
                    t0 = time.perf_counter()
                    capi._check(fn())
                    host.append(1e3 * (time.perf_counter() - t0))
                hip_ok(hip.hipEventRecord(ev[len(calls)], stream))
                hip_ok(hip.hipEventSynchronize(ev[len(calls)]))
                if rep:
                    for k, (key, _) in enumerate(calls):
                        t[key].append(elapsed(ev[k], ev[k + 1]))
                        if wall is not None:
                            wall.setdefault(key, []).append(host[k])
            for e in ev:
                hip.hipEventDestroy(e)
            return t

        say(f"\n## {name}; geom {geom} moves by 0.5 along x between the two views")
        check = {}
        it = [100]

        def render_one():
            it[0] += 1
            return L.pt_ctx_render(ctx, it[0], 1)

        for k in (1, 2):
            capi._check(L.pt_ctx_clear(ctx))
            capi._check(L.pt_ctx_render(ctx, 1, k))
            capi._check(L.pt_ctx_render_features(ctx, 1, 1))
            if k == 1:
                t = timed([("keep", lambda: L.pt_ctx_history_probe_keep(ctx, 1, 1, 0))])
                line("pt_history_probe_keep", t["keep"])
            capi._check(L.pt_ctx_history_probe_keep(ctx, 1, k, 0))
            capi._check(L.pt_ctx_history_capture_ex(ctx, C.c_float(k), MOM))
            trs = scene.geom_trs(geom)
            trs[0] += np.float32(0.5)
            scene.set_geom_trs(geom, trs)
            capi._check(L.pt_ctx_set_geoms(ctx, scene.desc.geoms, scene.desc.num_geoms))
            capi._check(L.pt_ctx_render(ctx, 10, k))
            capi._check(L.pt_ctx_render_features(ctx, 1, 1))
            wall = {}
            t = timed([("lookup", lambda: L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), MOM | MOTION)),
                       ("check", lambda: L.pt_ctx_history_probe_check(ctx, C.byref(popt), C.byref(probes), C.byref(changed), C.byref(skipped))),
                       ("render", render_one)], wall)
            say(f"### {k} iteration(s) per view: {changed.value} of {probes.value} probes changed, {skipped.value} skipped")
            line("pt_history_reproject_ex (motion)", t["lookup"])
            check[k] = line(f"pt_history_probe_check, k = {k}", t["check"])
            say(f"    that call on the host, median {statistics.median(wall['check']):.4f} ms (it ends in the one synchronise)")
            line("pt_render, 1 iteration", t["render"])
        replay = check[2] - check[1]
        say(f"### by difference: one replayed iteration of {probes.value} pixels {replay:.4f} ms; list + gradient + apply (and the first iteration's camera "
            f"rays) at most {check[1] - replay:.4f} ms")
    finally:
        L.pt_ctx_destroy(ctx)
out.close()
