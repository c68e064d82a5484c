#!/usr/bin/env python3
"""What editing a material of a live renderer costs (pt_set_materials) against pt_free + pt_init, and what the lookup with
PT_HISTORY_MATERIALS costs beside the lookup without it and beside the motion lookup; profiles/set_materials_cost.log is this tool's
output.

  tools/set_materials_cost.py [--reps 21] [--log FILE]

Cornell and the 10,170-primitive stress scene at 1920 x 1080, fast arithmetic.  Part 1: a fresh pt_init, three pt_set_materials calls
that each recolour material 2 a step and dim the light a step, with four iterations after each, and as the baseline pt_free + pt_init
with the materials the last call left, in the same process.  Host wall clock (time.perf_counter around the calls through ctypes) next
to the library's own PtSetMaterialsTimes (upload / re-arm) and PtSetupTimes.  One run, nothing averaged.
Part 2, one context, per kind (plain, variance, moments): a view is rendered, its first hits are taken and captured; then
pt_set_materials recolours material 2 and pt_set_geoms moves geom 6, the next view is rendered, and per repetition the lookup without
a flag, with PT_HISTORY_MOTION and with PT_HISTORY_MATERIALS run back to back between HIP events on the context's stream.  Medians of
--reps - 1 times (the first repetition, which builds and uploads the tables, is dropped and the host wall time of its flagged call
printed).  No timing is asserted anywhere."""
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
WALL, LIGHT = 2, 0
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


def edit(scene, step=0.0625):
    m = scene.material(WALL)
    m.color[2] = float(np.float32(m.color[2]) + np.float32(step))
    scene.set_material(WALL, m)
    m = scene.material(LIGHT)
    m.emittance = float(np.float32(m.emittance) - np.float32(step))
    scene.set_material(LIGHT, m)


SCENES = (("cornell (7 primitives)", scenes.cornell_scene_text(res=(W, H))), ("stress 22x22x21 (10170 primitives)", scenes.stress_scene_text()))
tmp = tempfile.mkdtemp()
say(f"# pt_set_materials against pt_free + pt_init, MI355X, {W} x {H}, fast arithmetic; host wall clock (time.perf_counter around the call through")
say("# ctypes) and PtSetMaterialsTimes / PtSetupTimes (std::chrono::steady_clock inside the library); one run, no repetitions averaged")
for name, text in SCENES:
    path = scenes.write_scene(text, os.path.join(tmp, "s.txt"))
    say(f"\n## {name}")
    scene = capi.Scene(path)
    t0 = time.perf_counter()
    r = capi.Renderer(scene, arith="fast")
    wall = ms(t0)
    t, st = r.setup_times(), r.stats()
    say(f"fresh pt_init                             {wall:9.3f} ms wall   (tables {t.tables_ms:.3f}, upload {t.upload_ms:.3f}, buffers {t.buffers_ms:.3f}, "
        f"probe {t.probe_ms:.3f} ms; device MB {st.device_bytes / 2**20:.1f})")
    r.render(1, 4)
    r.sync()
    for step in range(3):
        edit(scene)
        t0 = time.perf_counter()
        r.set_materials(scene)
        wall = ms(t0)
        g = r.set_materials_times()
        say(f"pt_set_materials, step {step + 1}                   {wall:9.3f} ms wall   (upload {g.upload_ms:.3f}, re-arm {g.rearm_ms:.3f}, total {g.total_ms:.3f} ms)")
        t0 = time.perf_counter()
        r.render(1, 4)
        r.sync()
        say(f"  4 iterations after it                   {ms(t0):9.3f} ms wall")
    t0 = time.perf_counter()
    r.free()
    freed = ms(t0)
    t0 = time.perf_counter()
    r = capi.Renderer(scene, arith="fast")  # the baseline: a fresh renderer with the materials the last call left
    wall = ms(t0)
    t = r.setup_times()
    say(f"pt_free + pt_init with those materials    {freed + wall:9.3f} ms wall   (free {freed:.3f}, init {wall:.3f}: tables {t.tables_ms:.3f}, upload "
        f"{t.upload_ms:.3f}, buffers {t.buffers_ms:.3f}, probe {t.probe_ms:.3f} ms)")
    r.free()

# ---- part 2: the lookup with PT_HISTORY_MATERIALS beside the lookup without it and the motion lookup -------------------------------
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
    say(f"{what:52s} median {statistics.median(v):8.4f} ms  min {v[0]:8.4f}  max {v[-1]:8.4f}  (n={len(v)})")


L = capi.lib()
L.pt_ctx_stream.argtypes = [C.c_void_p]
L.pt_ctx_stream.restype = C.c_void_p
MOTION, MATERIALS = capi.HISTORY_MOTION, capi.HISTORY_MATERIALS
say(f"\n# the lookup with PT_HISTORY_MATERIALS, one context, {W} x {H}, fast arithmetic; HIP events on the context's stream; {args.reps} repetitions, the first dropped")
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
        for label, kind in (("plain", 0), ("variance", capi.HISTORY_VARIANCE), ("moments", capi.HISTORY_MOMENTS)):
            def view():
                global first
                if kind == capi.HISTORY_VARIANCE:  # two folds
                    for _ in range(2):
                        capi._check(L.pt_ctx_render(ctx, first, SPP // 2))
                        capi._check(L.pt_ctx_noise_fold(ctx))
                        first += SPP // 2
                else:
                    capi._check(L.pt_ctx_render(ctx, first, SPP))
                    first += SPP
                capi._check(L.pt_ctx_render_features(ctx, 1, 1))

            capi._check(L.pt_ctx_clear(ctx))
            view()
            capi._check(L.pt_ctx_history_capture_ex(ctx, C.c_float(SPP), kind))
            edit(scene)
            capi._check(L.pt_ctx_set_materials(ctx, scene.desc.materials, scene.desc.num_materials))
            trs = scene.geom_trs(6)
            trs[0] += np.float32(0.0625)
            scene.set_geom_trs(6, trs)
            capi._check(L.pt_ctx_set_geoms(ctx, scene.desc.geoms, n))
            view()
            ev = [C.c_void_p() for _ in range(4)]
            for e in ev:
                hip_ok(hip.hipEventCreate(C.byref(e)))
            times = dict(plain=[], motion=[], materials=[])
            first_wall = 0.0
            for rep in range(args.reps):
                hip_ok(hip.hipEventRecord(ev[0], stream))
                capi._check(L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), kind))
                hip_ok(hip.hipEventRecord(ev[1], stream))
                capi._check(L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), kind | MOTION))
                hip_ok(hip.hipEventRecord(ev[2], stream))
                t0 = time.perf_counter()
                capi._check(L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), kind | MATERIALS))
                if rep == 0:
                    first_wall = ms(t0)
                hip_ok(hip.hipEventRecord(ev[3], stream))
                hip_ok(hip.hipEventSynchronize(ev[3]))
                if rep:
                    times["plain"].append(elapsed(ev[0], ev[1]))
                    times["motion"].append(elapsed(ev[1], ev[2]))
                    times["materials"].append(elapsed(ev[2], ev[3]))
            for e in ev:
                hip.hipEventDestroy(e)
            say(f"### {label}: the first call with PT_HISTORY_MATERIALS (table of {17 * n} bytes built, uploaded after a synchronise) {first_wall:.3f} ms host wall")
            line(f"pt_history_reproject_ex, {label}", times["plain"])
            line(f"pt_history_reproject_ex, {label} | PT_HISTORY_MOTION", times["motion"])
            line(f"pt_history_reproject_ex, {label} | PT_HISTORY_MATERIALS", times["materials"])
    finally:
        L.pt_ctx_destroy(ctx)
out.close()
