#!/usr/bin/env python3
"""What moving an object of a live renderer costs (pt_set_geoms) against pt_free + pt_init, and what the lookup with
PT_HISTORY_MOTION costs beside the lookup without it; profiles/set_geoms_cost.log is this tool's output.

  tools/set_geoms_cost.py [--reps 21] [--log FILE]

Cornell and the 10,170-primitive stress scene at 1920 x 1080.  Part 1, exact and fast arithmetic: a fresh pt_init, three pt_set_geoms
calls that each move one object a step (geom 6: cornell's sphere, the stress scene's first small object) with four iterations after
each, and as the baseline pt_free + pt_init with the geoms the last call left, in the same process.  Host wall clock
(time.perf_counter around the calls through ctypes) next to the library's own PtSetGeomsTimes (build / upload / re-arm) and
PtSetupTimes.  One run, nothing averaged.
Part 2, fast arithmetic, one context: a view is rendered (4 iterations), its first hits are taken and captured; then pt_set_geoms
moves ONE geom, the next view is rendered, and per repetition the lookup without the flag and the lookup with PT_HISTORY_MOTION run
back to back between HIP events on the context's stream; then the same with EVERY geom moved (each by the same small step).  Medians
of --reps - 1 times (the first repetition, which uploads the motion table, is dropped and its host wall time printed).  No timing is
asserted anywhere."""
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

W, H, SPP = 1920, 1080, 4
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


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def step_geom(scene, geom, dx):
    trs = scene.geom_trs(geom)
    trs[0] += np.float32(dx)
    scene.set_geom_trs(geom, trs)


SCENES = (("cornell (7 primitives)", scenes.cornell_scene_text(res=(W, H))), ("stress 22x22x21 (10170 primitives)", scenes.stress_scene_text()))
tmp = tempfile.mkdtemp()
say(f"# pt_set_geoms against pt_free + pt_init, MI355X, {W} x {H}; host wall clock (time.perf_counter around the call through ctypes) and")
say("# PtSetGeomsTimes / PtSetupTimes (std::chrono::steady_clock inside the library); one run, no repetitions averaged")
for name, text in SCENES:
    path = scenes.write_scene(text, os.path.join(tmp, "s.txt"))
    say(f"\n## {name}")
    for arith in ("exact", "fast"):
        scene = capi.Scene(path)
        t0 = time.perf_counter()
        r = capi.Renderer(scene, arith=arith)
        wall = ms(t0)
        t, st = r.setup_times(), r.stats()
        say(f"[{arith}] fresh pt_init                    {wall:9.3f} ms wall   (tables {t.tables_ms:.3f}, upload {t.upload_ms:.3f}, buffers {t.buffers_ms:.3f}, "
            f"probe {t.probe_ms:.3f} ms; grid_cells {st.grid_cells}, device MB {st.device_bytes / 2**20:.1f})")
        r.render(1, 4)
        r.sync()
        for step in range(3):
            step_geom(scene, 6, 0.25)
            t0 = time.perf_counter()
            r.set_geoms(scene)
            wall = ms(t0)
            g, st = r.set_geoms_times(), r.stats()
            say(f"[{arith}] pt_set_geoms, step {step + 1}              {wall:9.3f} ms wall   (build {g.build_ms:.3f}, upload {g.upload_ms:.3f}, re-arm {g.rearm_ms:.3f}, "
                f"total {g.total_ms:.3f} ms; grid_cells {st.grid_cells})")
            t0 = time.perf_counter()
            r.render(1, 4)
            r.sync()
            say(f"[{arith}]   4 iterations after it          {ms(t0):9.3f} ms wall")
        t0 = time.perf_counter()
        r.free()
        freed = ms(t0)
        t0 = time.perf_counter()
        r = capi.Renderer(scene, arith=arith)  # the baseline: a fresh renderer with the geoms the last call left
        wall = ms(t0)
        t = r.setup_times()
        say(f"[{arith}] pt_free + pt_init with those geoms {freed + wall:9.3f} ms wall   (free {freed:.3f}, init {wall:.3f}: tables {t.tables_ms:.3f}, upload "
            f"{t.upload_ms:.3f}, buffers {t.buffers_ms:.3f}, probe {t.probe_ms:.3f} ms)")
        t0 = time.perf_counter()
        r.render(1, 4)
        r.sync()
        say(f"[{arith}]   4 iterations after it          {ms(t0):9.3f} ms wall")
        r.free()

# ---- part 2: the lookup with PT_HISTORY_MOTION beside the lookup without it ----------------------------------------------------------
hip = C.CDLL("libamdhip64.so")
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
hip.hipEventDestroy.argtypes = [C.c_void_p]


def hip_ok(rc):
    if rc != 0:
        raise RuntimeError(f"HIP error {rc}")


def elapsed(a, b):
    t = C.c_float(0)
    hip_ok(hip.hipEventElapsedTime(C.byref(t), a, b))
    return float(t.value)


def line(what, v):
    v = sorted(v)
    say(f"{what:44s} median {statistics.median(v):8.4f} ms  min {v[0]:8.4f}  max {v[-1]:8.4f}  (n={len(v)})")


L = capi.lib()
L.pt_ctx_stream.argtypes = [C.c_void_p]
L.pt_ctx_stream.restype = C.c_void_p
MOTION = capi.HISTORY_MOTION
say(f"\n# the lookup with PT_HISTORY_MOTION, one context, {W} x {H}, fast arithmetic; HIP events on the context's stream; {args.reps} repetitions, the first dropped")
for name, text in SCENES:
    path = scenes.write_scene(text, os.path.join(tmp, "s.txt"))
    scene = capi.Scene(path, res=(W, H))
    n = scene.desc.num_geoms
    opt = capi.make_options(arith="fast")
    ctx = C.c_void_p()
    capi._check(L.pt_ctx_create(C.byref(scene.desc), C.byref(opt), C.byref(ctx)))
    try:
        stream = L.pt_ctx_stream(ctx)
        hopt = capi.history_options()
        say(f"\n## {name}")
        first = 1
        for label, moved in (("one geom moved", [6]), (f"all {n} geoms moved", list(range(n)))):
            capi._check(L.pt_ctx_render(ctx, first, SPP))
            capi._check(L.pt_ctx_render_features(ctx, 1, 1))
            capi._check(L.pt_ctx_history_capture(ctx, C.c_float(SPP)))
            for g in moved:
                step_geom(scene, g, 0.0625)
            capi._check(L.pt_ctx_set_geoms(ctx, scene.desc.geoms, n))
            first += SPP
            capi._check(L.pt_ctx_render(ctx, first, SPP))
            capi._check(L.pt_ctx_render_features(ctx, 1, 1))
            first += SPP
            ev = [C.c_void_p() for _ in range(3)]
            for e in ev:
                hip_ok(hip.hipEventCreate(C.byref(e)))
            times = dict(plain=[], motion=[])
            first_wall = 0.0
            for rep in range(args.reps):
                hip_ok(hip.hipEventRecord(ev[0], stream))
                capi._check(L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), 0))
                hip_ok(hip.hipEventRecord(ev[1], stream))
                t0 = time.perf_counter()
                capi._check(L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), MOTION))
                if rep == 0:
                    first_wall = ms(t0)
                hip_ok(hip.hipEventRecord(ev[2], stream))
                hip_ok(hip.hipEventSynchronize(ev[2]))
                if rep:
                    times["plain"].append(elapsed(ev[0], ev[1]))
                    times["motion"].append(elapsed(ev[1], ev[2]))
            for e in ev:
                hip.hipEventDestroy(e)
            cur = np.empty((W * H, 4), np.float32)
            capi._check(L.pt_ctx_readback_history(ctx, None, capi._f(cur)))
            say(f"### {label}: {int((cur[:, 3] > 0).sum())} of {W * H} pixels carried with the flag; the first call with it (table of {97 * n} bytes built, "
                f"uploaded after a synchronise) {first_wall:.3f} ms host wall")
            line("pt_history_reproject_ex, flags 0", times["plain"])
            line("pt_history_reproject_ex, PT_HISTORY_MOTION", times["motion"])
    finally:
        L.pt_ctx_destroy(ctx)
out.close()
