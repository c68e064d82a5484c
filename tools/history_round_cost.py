#!/usr/bin/env python3
"""What a history round costs (pt_history_round); profiles/history_round_cost.log is this tool's output.

  tools/history_round_cost.py [--reps 21] [--log FILE] [--json FILE]       one run with the library PT_AMD_LIB names (default: this tree's)
  tools/history_round_cost.py --compare PARENT1.json THIS.json PARENT2.json [--log FILE]

Cornell and the 10,170-primitive stress scene at 1920 x 1080, fast arithmetic, one context.  An orbit of 8 views 2 pi / 120 apart at 1
iteration per view is run through lookup, capture (with moments), and — where the library has it — a round of G = 3 after each lookup,
as the command line's --history-extra does.  At the 8th view, after its lookup, per repetition between HIP events on the context's
stream: pt_history_reproject and _reproject_ex, pt_history_resolve (device form), pt_history_denoise_ex (device form, E absent) and
ONE iteration of pt_render; then pt_history_capture and _capture_ex on their own.  These are the steps a library without the round has
too: --compare sets this library's medians beside those of two runs of the parent revision's (tools/build_rev.sh, PT_AMD_LIB) and says
which lie outside the spread of the parent's own two runs, and by how much.

Then the round, where the library has it.  Nothing is captured between the repetitions, so every one keys the same history and
selects the same pixels (E and S grow; the key reads neither).  The public call is one, so its parts are taken by difference:
  the whole round    the events around the call: key, select, the 8-byte readback, the worker's render of m pixels, the merge
  key + select       the events around a round in which nothing is fresh — after a capture the history is looked up standing still with
                     keep_view_dependent, so every hit pixel carries at least one sample, and min_history is 1e-30: the key kernel and
                     the selection's launches are the same whatever they select, and nothing else runs
  synchronise        that call's time on the host minus its time between the events: what the one wait costs beyond the kernels
  render + merge     the whole round minus key + select.  The merge is one launch of m threads behind the render on the same stream; the
                     public calls do not separate it
and the counted forms of resolve, filter and capture on the same frame, while E is present.
The first repetition (allocations, code objects) is dropped.  No timing is asserted anywhere."""
import argparse
import ctypes as C
import json
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
ap.add_argument("--json", default=None)
ap.add_argument("--compare", nargs=3, default=None)
args = ap.parse_args()
out = open(args.log, "a")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


if args.compare:
    p1, this, p2 = (json.load(open(f)) for f in args.compare)
    say("\n# the steps the parent revision has too: medians in ms — parent run 1, parent run 2, this library; 'outside' where this library's")
    say("# median lies outside the interval of the parent's two runs, with the distance to its nearer end")
    for scene in this:
        say(f"## {scene}")
        for step, v in this[scene].items():
            if step not in p1.get(scene, {}) or step not in p2.get(scene, {}):
                continue
            a, b = sorted((p1[scene][step], p2[scene][step]))
            where = "within the parent's spread" if a <= v <= b else f"outside by {(v - b if v > b else v - a):+.4f} ms ({100 * (v / (b if v > b else a) - 1):+.2f} %)"
            say(f"{step:30s} {p1[scene][step]:9.4f} {p2[scene][step]:9.4f} {v:9.4f}   {where}")
    sys.exit(0)

import numpy as np  # noqa: E402

from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes  # noqa: E402

W, H, G, VIEWS = 1920, 1080, 3, 8
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
have_round = hasattr(L, "pt_ctx_history_round")
MOM = capi.HISTORY_MOMENTS
medians = {}


def line(scene, what, v):
    v = sorted(v)
    med = statistics.median(v)
    medians.setdefault(scene, {})[what] = med
    say(f"{what:30s} median {med:9.4f} ms  min {v[0]:9.4f}  max {v[-1]:9.4f}  (n={len(v)})")
    return med


say(f"\n# library: {os.path.basename(os.environ.get('PT_AMD_LIB', '')) or 'this tree'}; the history round {'present' if have_round else 'absent'}; MI355X, {W} x {H}, fast arithmetic, "
    f"{args.reps} repetitions, the first dropped; the 8th view of an orbit at 1 iteration per view" + (f", rounds of {G} after every lookup" if have_round else ""))
tmp = tempfile.mkdtemp()
for name, text in (("cornell (7 primitives)", scenes.cornell_scene_text(res=(W, H))), ("stress 22x22x21 (10170 primitives)", scenes.stress_scene_text())):
    path = scenes.write_scene(text, os.path.join(tmp, "s.txt"))
    scene = capi.Scene(path, res=(W, H))
    opt = capi.make_options(arith="fast")
    ctx = C.c_void_p()
    capi._check(L.pt_ctx_create(C.byref(scene.desc), C.byref(opt), C.byref(ctx)))
    try:
        stream = L.pt_ctx_stream(ctx)
        hopt, one, dev = capi.history_options(), C.c_float(1.0), C.c_void_p()
        ropt = capi.PtHistoryRoundOptions(0.0, 0.0) if have_round else None
        fresh, m = C.c_int32(0), C.c_int32(0)
        moves = [0]

        def orbit(rounds):
            """VIEWS views up to the last one's lookup; rounds: a round of G after every lookup but the last, which is left to be timed."""
            per_view = []
            for f in range(VIEWS):
                if moves[0] > 0:
                    cam = scene.orbit(np.float32(2 * np.pi / 120), 0.0, 0.0)
                    capi._check(L.pt_ctx_set_camera(ctx, C.byref(cam)))
                moves[0] += 1
                capi._check(L.pt_ctx_render(ctx, moves[0] * (1 + G) + 1, 1))
                capi._check(L.pt_ctx_render_features(ctx, 1, 1))
                if f > 0:
                    capi._check(L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), MOM))
                if f < VIEWS - 1:
                    if rounds:
                        capi._check(L.pt_ctx_history_round(ctx, moves[0] * (1 + G) + 2, G, C.byref(ropt), C.byref(fresh), C.byref(m)))
                        per_view.append(m.value)
                    capi._check(L.pt_ctx_history_capture_ex(ctx, one, MOM))
            return per_view

        orbit(False)  # without rounds: what a library without them runs too, on the same history

        def timed(calls, wall=None):
            """calls: (name, function) run back to back per repetition between HIP events; the first repetition is dropped.  wall: a dict
            that receives the host's time per call, ms."""
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

        say(f"\n## {name}")
        it = [VIEWS * (1 + G) + 1]

        def render_one():
            it[0] += 1
            return L.pt_ctx_render(ctx, it[0], 1)

        # the steps every library has, E absent; the lookups last, so that C and VC are the moments kind's for what follows
        t = timed([("pt_history_reproject", lambda: L.pt_ctx_history_reproject(ctx, C.byref(hopt))),
                   ("pt_history_resolve (device)", lambda: L.pt_ctx_history_resolve_device(ctx, one, C.byref(dev))),
                   ("pt_history_reproject_ex", lambda: L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), MOM)),
                   ("pt_history_denoise_ex (dev.)", lambda: L.pt_ctx_history_denoise_ex_device(ctx, one, None, MOM, C.byref(dev))),
                   ("pt_render, 1 iteration", render_one)])
        for k, v in t.items():
            line(name, k, v)
        if have_round:
            # a second orbit from where the first ended, with a round after every lookup as the command line's --history-extra runs them
            capi._check(L.pt_ctx_history_drop(ctx))
            per_view = orbit(True)
            say(f"### an orbit with rounds of {G}: m per view {per_view}; the 8th view's round, timed:")
            wall = {}
            t = timed([("pt_history_round", lambda: L.pt_ctx_history_round(ctx, 5000, G, C.byref(ropt), C.byref(fresh), C.byref(m)))], wall)
            whole = line(name, f"pt_history_round, G = {G}", t["pt_history_round"])
            say(f"    fresh {fresh.value}, m {m.value} of {W * H} pixels ({100 * m.value / (W * H):.3f} %); the host's time per call, median "
                f"{statistics.median(wall['pt_history_round']):.4f} ms: the call returns once its merge is enqueued, so what it waits for is key + select")
            # the counted forms on the same frame: E is present now
            t = timed([("resolve, counted (device)", lambda: L.pt_ctx_history_resolve_device(ctx, one, C.byref(dev))),
                       ("denoise_ex, counted (dev.)", lambda: L.pt_ctx_history_denoise_ex_device(ctx, one, None, MOM, C.byref(dev)))])
            for k, v in t.items():
                line(name, k, v)
        if have_round:
            t = timed([("pt_history_capture_ex", lambda: L.pt_ctx_history_capture_ex(ctx, one, MOM))])
            line(name, "capture_ex, counted", t["pt_history_capture_ex"])
            # nothing fresh: K is this view's now; looked up standing still with keep_view_dependent, every hit pixel carries >= 1 sample
            still = capi.history_options(keep_view_dependent=True)
            capi._check(L.pt_ctx_history_reproject_ex(ctx, C.byref(still), MOM))
            tiny = capi.PtHistoryRoundOptions(1e-30, 0.0)
            wall = {}
            t = timed([("pt_history_round", lambda: L.pt_ctx_history_round(ctx, 6000, G, C.byref(tiny), C.byref(fresh), C.byref(m)))], wall)
            if m.value:
                say(f"    ({m.value} pixels carried nothing even so and were rendered: the figure below includes them)")
            select = line(name, "key + select (nothing fresh)", t["pt_history_round"])
            host = statistics.median(wall["pt_history_round"])
            say(f"    that call on the host, median {host:.4f} ms: the synchronise costs {host - select:.4f} ms beyond the kernels")
            say(f"    render + merge of the round above, by difference: {whole - select:.4f} ms")
        # the captures with E and C absent, the same state in every library
        capi._check(L.pt_ctx_clear(ctx))
        capi._check(L.pt_ctx_render(ctx, 1, 1))
        capi._check(L.pt_ctx_render_features(ctx, 1, 1))
        t = timed([("pt_history_capture", lambda: L.pt_ctx_history_capture(ctx, one)),
                   ("pt_history_capture_ex", lambda: L.pt_ctx_history_capture_ex(ctx, one, MOM))])
        line(name, "pt_history_capture", t["pt_history_capture"])
        line(name, "pt_history_capture_ex", t["pt_history_capture_ex"])
    finally:
        L.pt_ctx_destroy(ctx)
if args.json:
    json.dump(medians, open(args.json, "w"), indent=1)
out.close()
