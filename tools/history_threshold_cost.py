#!/usr/bin/env python3
"""What threshold rounds over the blend cost and buy (pt_history_round_threshold and the history steps with per-pixel counts;
DESIGN.md section 10); profiles/history_threshold_cost.log holds this tool's output, of this library between two runs of the parent
revision's (PT_AMD_LIB), which skip the steps the parent lacks.

  tools/history_threshold_cost.py [--reps 21] [--log FILE] [--label NAME]

tools/history_cost.py's three scenes at 1920 x 1080, fast arithmetic, one context.  A view is rendered in 4 groups of 1 with a fold
each and captured with variance, the camera moves one orbit step of 2 pi / 120, the features are taken, the history is looked up and the
view is rendered and folded the same way.  Per repetition every step runs between HIP events on the context's stream, each new step
beside its sibling; the first repetition (allocations, code objects) is dropped and median, minimum and maximum are printed.  A step
that synchronises (the estimates, the rounds) holds that synchronise in its time, as its sibling does.  First in the uniform state,
then — after a threshold round with nothing above, which enters the adaptive state and renders nothing — with the count plane read.
The round with nothing above is key, selection, 8 bytes and a synchronise: pt_history_round_threshold's less
pt_adaptive_round_threshold's is pass A and pass B less k_adaptive_key.

Last the orbit the feature exists for: 8 views 2 pi / 120 apart, at most 32 iteration numbers per view in groups of 4 and again in
groups of 2 (the two uniform groups every view starts with are its floor: 8 and 4 iterations), max_fraction
0.25, until at most a thousandth of the pixels is above, on the wall clock, one run each: pt_render_threshold per view without history
(with and without the features and pt_denoise_adaptive a filtered frame needs) against features, lookup, pt_history_render_threshold,
pt_history_denoise_adaptive and pt_history_capture_adaptive.  E is found at view 0: the square root of the 95th percentile of the
view's own estimate w after 16 uniform iterations in 4 folded groups — what uniform sampling meets in 95 % of the pixels at 16 spp.
No timing is asserted anywhere."""
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
N = W * H
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--log", default=os.devnull)
ap.add_argument("--label", default="the tree's library", help="what the log calls the library (PT_AMD_LIB chooses it)")
args = ap.parse_args()
out = open(args.log, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


hip = C.CDLL("libamdhip64.so")
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]


def hip_ok(rc):
    if rc != 0:
        raise RuntimeError(f"HIP error {rc}")


def line(what, v):
    v = sorted(v)
    say(f"{what:44s} median {statistics.median(v):8.4f} ms  min {v[0]:8.4f}  max {v[-1]:8.4f}  (n={len(v)})")
    return statistics.median(v)


L = capi.lib()
L.pt_ctx_stream.argtypes = [C.c_void_p]
L.pt_ctx_stream.restype = C.c_void_p
NEW = hasattr(L, "pt_ctx_history_round_threshold")  # False: the parent revision's library
VAR = capi.HISTORY_VARIANCE
say(f"# threshold rounds over the blend on one context, MI355X, {W} x {H}, fast arithmetic; HIP events on the context's stream; {args.reps} repetitions, "
    f"the first dropped; this library {'has' if NEW else 'lacks'} the new calls ({args.label})")
tmp = tempfile.mkdtemp()
for name, text in (("cornell (7 primitives)", scenes.cornell_scene_text(res=(W, H))), ("stress 22x22x21 (10170 primitives)", scenes.stress_scene_text()),
                   ("cornell from inside the box", scenes.cornell_scene_text(res=(W, H), eye=(0.0, 5.0, 4.5)))):
    path = scenes.write_scene(text, os.path.join(tmp, "s.txt"))
    scene = capi.Scene(path, res=(W, H))
    opt = capi.make_options(arith="fast")
    ctx = C.c_void_p()
    capi._check(L.pt_ctx_create(C.byref(scene.desc), C.byref(opt), C.byref(ctx)))
    try:
        stream = L.pt_ctx_stream(ctx)
        ev = [C.c_void_p(), C.c_void_p()]
        for e in ev:
            hip_ok(hip.hipEventCreate(C.byref(e)))
        dev, sse, hopt = C.c_void_p(), C.c_double(0.0), capi.history_options()
        above, selected = C.c_int32(0), C.c_int32(0)
        samples = C.c_float(SPP)

        def timed(steps):
            """steps: [(name, call)], run in that order every repetition; {name: [ms]} without the first repetition."""
            t = {k: [] for k, _ in steps}
            for rep in range(args.reps):
                for k, call in steps:
                    hip_ok(hip.hipEventRecord(ev[0], stream))
                    capi._check(call())
                    hip_ok(hip.hipEventRecord(ev[1], stream))
                    hip_ok(hip.hipEventSynchronize(ev[1]))
                    ms = C.c_float(0)
                    hip_ok(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
                    if rep:
                        t[k].append(float(ms.value))
            return t

        def folded_view(first):
            for g in range(SPP):
                capi._check(L.pt_ctx_render(ctx, first + g, 1))
                capi._check(L.pt_ctx_noise_fold(ctx))

        folded_view(1)
        capi._check(L.pt_ctx_render_features(ctx, 1, 1))
        capi._check(L.pt_ctx_history_capture_ex(ctx, samples, VAR))
        step = np.float32(2 * np.pi / 120)
        capi._check(L.pt_ctx_set_camera(ctx, C.byref(scene.orbit(step, 0.0, 0.0))))
        capi._check(L.pt_ctx_render_features(ctx, 1, 1))
        capi._check(L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), VAR))
        folded_view(SPP + 1)
        old = [("pt_history_noise", lambda: L.pt_ctx_history_noise(ctx, samples, VAR, C.byref(sse))),
               ("pt_history_resolve (device)", lambda: L.pt_ctx_history_resolve_device(ctx, samples, C.byref(dev))),
               ("pt_history_capture_ex", lambda: L.pt_ctx_history_capture_ex(ctx, samples, VAR)),
               ("pt_history_denoise (device)", lambda: L.pt_ctx_history_denoise_device(ctx, samples, None, C.byref(dev))),
               ("pt_denoise_adaptive (device)", lambda: L.pt_ctx_denoise_adaptive_device(ctx, None, C.byref(dev)))]
        new = [("pt_history_noise_adaptive", lambda: L.pt_ctx_history_noise_adaptive(ctx, C.byref(sse))),
               ("pt_history_resolve_adaptive (device)", lambda: L.pt_ctx_history_resolve_adaptive_device(ctx, C.byref(dev))),
               ("pt_history_capture_adaptive", lambda: L.pt_ctx_history_capture_adaptive(ctx)),
               ("pt_history_denoise_adaptive (device)", lambda: L.pt_ctx_history_denoise_adaptive_device(ctx, None, C.byref(dev)))] if NEW else []
        say(f"\n## {name}: a view with a carried history (C and VC present), the uniform state, counts (4, 4)")
        t = timed(old + new)
        med = {k: line(k, v) for k, v in t.items()}
        if NEW:
            for a, b in (("pt_history_noise_adaptive", "pt_history_noise"), ("pt_history_resolve_adaptive (device)", "pt_history_resolve (device)"),
                         ("pt_history_capture_adaptive", "pt_history_capture_ex"), ("pt_history_denoise_adaptive (device)", "pt_history_denoise (device)"),
                         ("pt_history_denoise_adaptive (device)", "pt_denoise_adaptive (device)")):
                say(f"{a} / {b}: {med[a] / med[b]:.3f}")
        # the adaptive state: a round with nothing above enters it and renders nothing
        nothing = C.c_float(1e3)
        rounds = [("pt_adaptive_round_threshold, nothing above", lambda: L.pt_ctx_adaptive_round_threshold(ctx, 100, 1, nothing, C.c_float(0.25), C.byref(above), C.byref(selected)))]
        if NEW:
            rounds.append(("pt_history_round_threshold, nothing above", lambda: L.pt_ctx_history_round_threshold(ctx, 100, 1, nothing, C.c_float(0.25), C.byref(above), C.byref(selected))))
        say("### the adaptive state (the count plane is read): key, selection, 8 bytes and a synchronise; then the steps again")
        t = timed(rounds + [old[4]] + new)
        assert above.value == 0 and selected.value == 0
        med = {k: line(k, v) for k, v in t.items()}
        if NEW:
            say(f"pt_history_round_threshold less pt_adaptive_round_threshold (pass A and pass B less k_adaptive_key): "
                f"{med['pt_history_round_threshold, nothing above'] - med['pt_adaptive_round_threshold, nothing above']:+.4f} ms")
            say(f"pt_history_denoise_adaptive / pt_denoise_adaptive: {med['pt_history_denoise_adaptive (device)'] / med['pt_denoise_adaptive (device)']:.3f}")
        # ---- the orbit
        CAP, VIEWS, FRACTION, MIN_PIXELS = 32, 8, C.c_float(0.25), N // 1000
        fresh = capi.Scene(path, res=(W, H))
        cams = [fresh.camera] + [fresh.orbit(step, 0.0, 0.0) for _ in range(VIEWS - 1)]
        capi._check(L.pt_ctx_history_drop(ctx))
        capi._check(L.pt_ctx_set_camera(ctx, C.byref(cams[0])))
        for g in range(4):
            capi._check(L.pt_ctx_render(ctx, 1 + 4 * g, 4))
            capi._check(L.pt_ctx_noise_fold(ctx))
        planes = np.empty((capi.NOISE_PLANES, N, 4), np.float32)
        capi._check(L.pt_ctx_readback_noise(ctx, capi._f(planes)))
        E = C.c_float(float(np.sqrt(np.percentile(planes[0, :, 3].astype(np.float64), 95))))
        done, total, left = C.c_int32(0), C.c_int64(0), C.c_int32(0)
        rules = ["pt_render_threshold", "pt_render_threshold + features + pt_denoise_adaptive"] + (["pt_history_render_threshold + lookup, filter, capture"] if NEW else [])
        for G, rule in [(g, rule) for g in (4, 2) for rule in rules]:
            capi._check(L.pt_ctx_history_drop(ctx))
            capi._check(L.pt_ctx_sync(ctx))
            iters, samples_per_view, t0 = [], [], time.perf_counter()
            for f in range(VIEWS):
                capi._check(L.pt_ctx_set_camera(ctx, C.byref(cams[f])))
                if rule.startswith("pt_render_threshold"):
                    capi._check(L.pt_ctx_render_threshold(ctx, f * CAP + 1, CAP, G, E, FRACTION, MIN_PIXELS, C.byref(done), C.byref(total), C.byref(left)))
                    if "features" in rule:
                        capi._check(L.pt_ctx_render_features(ctx, 1, 1))
                        capi._check(L.pt_ctx_denoise_adaptive_device(ctx, None, C.byref(dev)))
                else:
                    capi._check(L.pt_ctx_render_features(ctx, 1, 1))
                    if f:
                        capi._check(L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), VAR))
                    capi._check(L.pt_ctx_history_render_threshold(ctx, f * CAP + 1, CAP, G, E, FRACTION, MIN_PIXELS, C.byref(done), C.byref(total), C.byref(left)))
                    capi._check(L.pt_ctx_history_denoise_adaptive_device(ctx, None, C.byref(dev)))
                    capi._check(L.pt_ctx_history_capture_adaptive(ctx))
                iters.append(done.value), samples_per_view.append(total.value)
            capi._check(L.pt_ctx_sync(ctx))
            say(f"orbit of {VIEWS} views, E {E.value:.5f}, cap {CAP}, groups of {G}, max_fraction 0.25, until {MIN_PIXELS} pixels, {rule}: "
                f"{1e3 * (time.perf_counter() - t0):9.2f} ms wall (moves included), iteration numbers per view {iters}, "
                f"samples {sum(samples_per_view)} = {sum(samples_per_view) / (VIEWS * CAP * N):.4f} of {CAP} uniform spp, per view in spp {[round(s / N, 2) for s in samples_per_view]}")
    finally:
        L.pt_ctx_destroy(ctx)
out.close()
