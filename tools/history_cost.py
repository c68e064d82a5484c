#!/usr/bin/env python3
"""What the reprojected sample history costs (pt_history_capture / _reproject / _resolve);
profiles/history_cost.log is this tool's output.

  tools/history_cost.py [--reps 21] [--log FILE]

Cornell and the 10,170-primitive stress scene at 1920 x 1080, fast arithmetic, one context.  A view is rendered (4 iterations), its
first hits are taken (pt_render_features(1, 1)) and captured; the camera moves one orbit step of 2 pi / 120; then, per repetition,
reproject, resolve (the device form: no readback) and capture run back to back on the context's stream between HIP events, and the
median, minimum and maximum of each are printed with the bytes a call moves by its specification (the gather's taps: 4 x 32 B read
at the most, 4 x 16 B more for taps that pass, before any cache) and the rate that makes.  The yardstick is one iteration of pt_render
at the same camera, in the same process, timed the same way.  The first repetition (allocations, code objects) is dropped.  No timing
is asserted anywhere.

Then the variance side (PT_HISTORY_VARIANCE; profiles/history_variance_cost.log holds a run with both parts): the context is
cleared, a view is rendered in 4 groups of 1 with a fold each and captured with variance, the camera moves another step, the next view
is rendered and folded the same way; per repetition pt_history_reproject_ex and pt_history_capture_ex with the flag and
pt_history_denoise (device form) run between HIP events, and pt_denoise_guided (device form) on the same frame for scale.  The
first part is untouched by this: its calls are the flags == 0 ones, to be compared with earlier logs.

Then the moments side (PT_HISTORY_MOMENTS; profiles/history_moments_cost.log holds a run with all three parts, of this library and of
the parent revision's through PT_AMD_LIB), on cornell as above — at 16 : 9 over half of its camera rays miss, and a miss is marked
at every view — and on cornell with the eye inside the box, where every ray hits: the context is cleared and a view of 1 iteration is rendered; per repetition
pt_history_denoise_ex (device form) runs with C absent — the first view: every pixel is marked and k_denoise_var_spatial walks 49 taps
for each — and pt_history_capture_ex with the flag.  Then an orbit of 8 views 2 pi / 120 apart is run through lookup, filter and
capture, and at its last view — a steady view — pt_history_reproject_ex and pt_history_denoise_ex are timed per repetition, beside
pt_denoise (device form) on the same frame for scale; nothing is captured between the repetitions, so each looks the same history
up and marks the same pixels, whose share is printed with the times.  pt_history_capture_ex is timed afterwards, on its own.

Then the feedback (PT_HISTORY_FEEDBACK; profiles/history_feedback_cost.log holds this library's run between two of the parent
revision's), on every scene, last, so that the steps above run as they ran: the same orbit of 8 views with the flag in lookup, filter
(pt_history_denoise_feedback, the library's defaults) and capture; at its last view, per repetition, the moments lookup and then the
lookup with the flag, pt_history_denoise_ex and then pt_history_denoise_feedback (device forms); then the filter and the capture with the
flag as a pair (a capture promotes the pending plane, so each needs a tap before it), and the moments capture alone.

Then the noise estimate of the blend (pt_history_noise, pt_history_render_until; profiles/history_noise_cost.log holds this library's run
between two of the parent revision's), last of all on every scene: a view with a carried history, and per repetition one iteration of
pt_render, pt_noise_fold, pt_get_noise (a synchronise and 8 bytes read back, no kernel) and pt_history_noise (whose time holds the same
synchronise and readback beside its two kernels); then one group of
the driver — an iteration and the fused launch — against those three.  Last an orbit of 8 views 2 pi / 120 apart, at most 16
iterations per view in groups of 1, timed on the wall clock under pt_render_until and under pt_history_render_until (features, lookups
and captures included) with the iterations each took; the target is the estimate view 0 alone shows after 8 iterations."""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile

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


def line(what, v, bytes_per_pixel=None):
    v = sorted(v)
    med = statistics.median(v)
    rate = f"  {bytes_per_pixel} B/pixel by specification = {bytes_per_pixel * W * H / med / 1e6:7.1f} GB/s at the median" if bytes_per_pixel else ""
    say(f"{what:28s} median {med:8.4f} ms  min {v[0]:8.4f}  max {v[-1]:8.4f}  (n={len(v)}){rate}")


L = capi.lib()
L.pt_ctx_stream.argtypes = [C.c_void_p]
L.pt_ctx_stream.restype = C.c_void_p
say(f"# pt_history_* on one context, MI355X, {W} x {H}, fast arithmetic; HIP events on the context's stream; {args.reps} repetitions, the first dropped")
say("# per repetition: reproject, resolve, capture, then ONE iteration of pt_render (the yardstick), so every history call follows a render")
say("# the rates are bytes by specification over time, not memory traffic: where one exceeds what HBM delivers (about 6.3 TB/s measured on")
say("# this chip), the caches served part of it - the history's planes, the feature planes, S and the output are about 280 MB at this size,")
say("# the Infinity Cache holds 256 MiB, and the gather's four taps share lines between neighbouring pixels")
tmp = tempfile.mkdtemp()
# (the third: the eye inside the box, so that every camera ray hits — a miss carries no history and is marked at every view)
for name, text in (("cornell (7 primitives)", scenes.cornell_scene_text(res=(W, H))), ("stress 22x22x21 (10170 primitives)", scenes.stress_scene_text()),
                   ("cornell from inside the box", scenes.cornell_scene_text(res=(W, H), eye=(0.0, 5.0, 4.5)))):
    path = scenes.write_scene(text, os.path.join(tmp, "s.txt"))
    scene = capi.Scene(path, res=(W, H))
    opt = capi.make_options(arith="fast")
    ctx = C.c_void_p()
    capi._check(L.pt_ctx_create(C.byref(scene.desc), C.byref(opt), C.byref(ctx)))
    try:
        stream = L.pt_ctx_stream(ctx)
        st = capi.PtStats()
        capi._check(L.pt_ctx_get_stats(ctx, C.byref(st)))
        before = st.device_bytes
        capi._check(L.pt_ctx_render(ctx, 1, SPP))
        capi._check(L.pt_ctx_render_features(ctx, 1, 1))
        capi._check(L.pt_ctx_history_capture(ctx, C.c_float(SPP)))
        cam = scene.orbit(np.float32(2 * np.pi / 120), 0.0, 0.0)
        capi._check(L.pt_ctx_set_camera(ctx, C.byref(cam)))
        capi._check(L.pt_ctx_render(ctx, SPP + 1, SPP))
        capi._check(L.pt_ctx_render_features(ctx, 1, 1))
        times = dict(reproject=[], resolve=[], capture=[], render=[])
        ev = events(6)
        dev = C.c_void_p()
        hopt = capi.history_options()
        for rep in range(args.reps):
            hip_ok(hip.hipEventRecord(ev[0], stream))
            capi._check(L.pt_ctx_history_reproject(ctx, C.byref(hopt)))
            hip_ok(hip.hipEventRecord(ev[1], stream))
            capi._check(L.pt_ctx_history_resolve_device(ctx, C.c_float(SPP), C.byref(dev)))
            hip_ok(hip.hipEventRecord(ev[2], stream))
            capi._check(L.pt_ctx_history_capture(ctx, C.c_float(SPP)))
            hip_ok(hip.hipEventRecord(ev[3], stream))
            hip_ok(hip.hipEventRecord(ev[4], stream))
            capi._check(L.pt_ctx_render(ctx, 2 * SPP + 1 + rep, 1))
            hip_ok(hip.hipEventRecord(ev[5], stream))
            hip_ok(hip.hipEventSynchronize(ev[5]))
            if rep:
                times["reproject"].append(elapsed(ev[0], ev[1]))
                times["resolve"].append(elapsed(ev[1], ev[2]))
                times["capture"].append(elapsed(ev[2], ev[3]))
                times["render"].append(elapsed(ev[4], ev[5]))
        for e in ev:
            hip.hipEventDestroy(e)
        kept = np.empty((capi.HISTORY_KEPT_PLANES, W * H, 4), np.float32)
        cur = np.empty((W * H, 4), np.float32)
        capi._check(L.pt_ctx_readback_history(ctx, capi._f(kept), capi._f(cur)))
        capi._check(L.pt_ctx_get_stats(ctx, C.byref(st)))
        carried = cur[:, 3] > 0
        say(f"\n## {name}: {int(carried.sum())} of {W * H} pixels carried after the step, mean weight {float(cur[carried, 3].mean()) if carried.any() else 0.0:.2f}; "
            f"state {(st.device_bytes - before) / 2**20:.1f} MB (history planes, reject table, the resolve's buffer, the feature planes)")
        line("pt_history_reproject", times["reproject"], 48 + 16 + 4 * 48)
        line("pt_history_resolve (device)", times["resolve"], 12 + 16 + 12)
        line("pt_history_capture", times["capture"], 12 + 48 + 16 + 48)
        line("pt_render, 1 iteration", times["render"])
        three = statistics.median(times["reproject"]) + statistics.median(times["resolve"]) + statistics.median(times["capture"])
        say(f"the three together {three:.4f} ms = {three / statistics.median(times['render']):.3f} of one iteration")
        have = hasattr(L, "pt_ctx_history_denoise_device")  # False: an older build of the library (PT_AMD_LIB), which gives pt_denoise_guided's time
        # ---- the variance side: the same context, cleared; views folded in 4 groups of 1
        capi._check(L.pt_ctx_get_stats(ctx, C.byref(st)))
        before = st.device_bytes
        capi._check(L.pt_ctx_clear(ctx))
        VAR = capi.HISTORY_VARIANCE

        def folded_view(first):
            for g in range(SPP):
                capi._check(L.pt_ctx_render(ctx, first + g, 1))
                capi._check(L.pt_ctx_noise_fold(ctx))
            capi._check(L.pt_ctx_render_features(ctx, 1, 1))

        folded_view(1)
        if have:
            capi._check(L.pt_ctx_history_capture_ex(ctx, C.c_float(SPP), VAR))
        cam = scene.orbit(np.float32(2 * np.pi / 120), 0.0, 0.0)
        capi._check(L.pt_ctx_set_camera(ctx, C.byref(cam)))
        folded_view(SPP + 1)
        times = dict(reproject=[], denoise=[], capture=[], guided=[])
        ev = events(5)
        for rep in range(args.reps):
            hip_ok(hip.hipEventRecord(ev[0], stream))
            if have:
                capi._check(L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), VAR))
            hip_ok(hip.hipEventRecord(ev[1], stream))
            if have:
                capi._check(L.pt_ctx_history_denoise_device(ctx, C.c_float(SPP), None, C.byref(dev)))
            hip_ok(hip.hipEventRecord(ev[2], stream))
            capi._check(L.pt_ctx_denoise_guided_device(ctx, None, C.byref(dev)))
            hip_ok(hip.hipEventRecord(ev[3], stream))
            if have:
                capi._check(L.pt_ctx_history_capture_ex(ctx, C.c_float(SPP), VAR))
            hip_ok(hip.hipEventRecord(ev[4], stream))
            hip_ok(hip.hipEventSynchronize(ev[4]))
            if rep:
                for k, name_ in enumerate(("reproject", "denoise", "guided", "capture")):
                    times[name_].append(elapsed(ev[k], ev[k + 1]))
        for e in ev:
            hip.hipEventDestroy(e)
        capi._check(L.pt_ctx_get_stats(ctx, C.byref(st)))
        if not have:
            say("### this build of the library has no PT_HISTORY_VARIANCE: the guided filter on the same frame, for scale")
            line("pt_denoise_guided (device)", times["guided"])
            continue
        say(f"### with PT_HISTORY_VARIANCE: {(st.device_bytes - before) / 2**20:.1f} MB more state (VK and VC, the fold's planes, the filters' workspace)")
        line("pt_history_reproject_ex", times["reproject"], 48 + 16 + 16 + 4 * 64)
        line("pt_history_capture_ex", times["capture"], 12 + 48 + 16 + 48 + 32 + 16 + 16)
        line("pt_history_denoise (device)", times["denoise"])
        line("pt_denoise_guided (device)", times["guided"])
        extra = statistics.median(times["denoise"]) - statistics.median(times["guided"])
        say(f"the history form's prepare reads 12 + 48 + 32 + 16 + 16 B and writes 64 B per pixel (the guided form's: 12 + 48 + 32 in); the two filters differ by {extra:+.4f} ms")
        history_denoise_median = statistics.median(times["denoise"])
        # ---- the moments side: the same context, cleared; views of 1 iteration, no fold
        if not hasattr(L, "pt_ctx_history_denoise_ex_device"):
            say("### this build of the library has no PT_HISTORY_MOMENTS")
            continue
        MOM = capi.HISTORY_MOMENTS
        one = C.c_float(1.0)

        def timed(calls):
            """calls: (name, function) run back to back per repetition between HIP events; the first repetition is dropped."""
            ev = events(len(calls) + 1)
            t = {k: [] for k, _ in calls}
            for rep in range(args.reps):
                for k, (_, fn) in enumerate(calls):
                    hip_ok(hip.hipEventRecord(ev[k], stream))
                    capi._check(fn())
                hip_ok(hip.hipEventRecord(ev[len(calls)], stream))
                hip_ok(hip.hipEventSynchronize(ev[len(calls)]))
                if rep:
                    for k, (key, _) in enumerate(calls):
                        t[key].append(elapsed(ev[k], ev[k + 1]))
            for e in ev:
                hip.hipEventDestroy(e)
            return t

        def feedback_part():
            """The feedback, last on every scene: the orbit of 8 views with the flag, then the steady view's steps beside the moments kind's."""
            if not hasattr(L, "pt_ctx_history_denoise_feedback_device"):
                say("### this build of the library has no PT_HISTORY_FEEDBACK")
                return
            FB = MOM | capi.HISTORY_FEEDBACK
            capi._check(L.pt_ctx_get_stats(ctx, C.byref(st)))
            before = st.device_bytes
            capi._check(L.pt_ctx_history_drop(ctx))
            capi._check(L.pt_ctx_clear(ctx))
            for f in range(8):
                if f:
                    cam = scene.orbit(np.float32(2 * np.pi / 120), 0.0, 0.0)
                    capi._check(L.pt_ctx_set_camera(ctx, C.byref(cam)))
                capi._check(L.pt_ctx_render(ctx, f + 1, 1))
                capi._check(L.pt_ctx_render_features(ctx, 1, 1))
                if f:
                    capi._check(L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), FB))
                if f < 7:
                    capi._check(L.pt_ctx_history_denoise_feedback_device(ctx, one, None, None, C.byref(dev)))
                    capi._check(L.pt_ctx_history_capture_ex(ctx, one, FB))
            t = timed([("moments lookup", lambda: L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), MOM)),
                       ("lookup", lambda: L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), FB)),
                       ("moments filter", lambda: L.pt_ctx_history_denoise_ex_device(ctx, one, None, MOM, C.byref(dev))),
                       ("filter", lambda: L.pt_ctx_history_denoise_feedback_device(ctx, one, None, None, C.byref(dev)))])
            t.update(timed([("filter before a capture", lambda: L.pt_ctx_history_denoise_feedback_device(ctx, one, None, None, C.byref(dev))),
                            ("capture", lambda: L.pt_ctx_history_capture_ex(ctx, one, FB))]))
            t.update(timed([("moments capture", lambda: L.pt_ctx_history_capture_ex(ctx, one, MOM))]))
            capi._check(L.pt_ctx_get_stats(ctx, C.byref(st)))
            say(f"### with PT_HISTORY_FEEDBACK, a steady view (the 8th of an orbit, 1 iteration each): {(st.device_bytes - before) / 2**20:.1f} MB more state (FK, FC, P)")
            line("reproject_ex, moments", t["moments lookup"], 48 + 16 + 16 + 4 * 64)
            line("reproject_ex, + feedback", t["lookup"], 48 + 16 + 16 + 16 + 4 * 80)
            line("pt_history_denoise_ex (dev.)", t["moments filter"])
            line("denoise_feedback (dev.)", t["filter"])
            line("capture_ex, moments", t["moments capture"], 12 + 48 + 16 + 48 + 16 + 16)
            line("capture_ex, + feedback", t["capture"], 12 + 48 + 16 + 48 + 16 + 16)
            say(f"the lookup with the flag against the moments lookup: {statistics.median(t['lookup']) - statistics.median(t['moments lookup']):+.4f} ms (16 B more out, "
                f"16 B more per tap that passed); the feedback filter against pt_history_denoise_ex: "
                f"{statistics.median(t['filter']) - statistics.median(t['moments filter']):+.4f} ms (the tap, 48 B per pixel, and 16 B per pixel more in prepare)")

        def noise_part():
            """The noise estimate of the blend and its driver, after everything else on every scene: the steps, then an orbit's wall time."""
            if not hasattr(L, "pt_ctx_history_noise"):
                say("### this build of the library has no pt_history_noise")
                return
            import time
            capi._check(L.pt_ctx_get_stats(ctx, C.byref(st)))
            before = st.device_bytes
            step = np.float32(2 * np.pi / 120)
            done, psnr, view, sse = C.c_int32(0), C.c_float(-1.0), C.c_float(-1.0), C.c_double(-1.0)
            count = [0]  # iterations the image holds

            def start_view(move):
                if move:
                    cam = scene.orbit(step, 0.0, 0.0)
                    capi._check(L.pt_ctx_set_camera(ctx, C.byref(cam)))
                else:
                    capi._check(L.pt_ctx_clear(ctx))
                capi._check(L.pt_ctx_render_features(ctx, 1, 1))
                count[0] = 0

            def one(first=1000):
                count[0] += 1
                return L.pt_ctx_render(ctx, first + count[0], 1)

            capi._check(L.pt_ctx_history_drop(ctx))
            start_view(False)
            for g in range(SPP):
                capi._check(one() or L.pt_ctx_noise_fold(ctx))
            capi._check(L.pt_ctx_history_capture_ex(ctx, C.c_float(SPP), VAR))
            start_view(True)
            capi._check(L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), VAR))
            for g in range(2):
                capi._check(one() or L.pt_ctx_noise_fold(ctx))
            # (pt_get_noise launches nothing: a synchronise and 8 bytes read back, what pt_history_noise's time holds beside its kernels)
            t = timed([("render", one), ("fold", lambda: L.pt_ctx_noise_fold(ctx)), ("sync", lambda: L.pt_ctx_get_noise(ctx, C.byref(sse), None, None)),
                       ("noise", lambda: L.pt_ctx_history_noise(ctx, C.c_float(count[0]), VAR, C.byref(sse)))])

            def fused():
                count[0] += 1
                return L.pt_ctx_history_render_until(ctx, 1000 + count[0], 1, 1, C.c_float(1000.0), None, None, None)

            t.update(timed([("fused step", fused)]))
            capi._check(L.pt_ctx_get_stats(ctx, C.byref(st)))
            say(f"### the noise estimate of the blend, a view with history (C and VC present): {(st.device_bytes - before) / 2**20:.1f} MB more state (W and the partial sums)")
            line("pt_render, 1 iteration", t["render"])
            line("pt_noise_fold", t["fold"], 12 + 32 + 32)
            line("pt_get_noise (a sync, 8 B)", t["sync"])
            line("pt_history_noise (with its sync)", t["noise"], 32 + 32 + 4)
            say(f"pt_history_noise less pt_get_noise's synchronise and readback: {statistics.median(t['noise']) - statistics.median(t['sync']):.4f} ms for k_history_noise and "
                f"the reduction, beside the fold's {statistics.median(t['fold']):.4f} ms for k_noise_fold and the same reduction")
            line("render + fused fold/estimate", t["fused step"])
            sep = statistics.median(t["render"]) + statistics.median(t["fold"]) + statistics.median(t["noise"])
            say(f"one group of the driver (an iteration, k_noise_fold_history, two reductions, 16 B read back) against the three separate steps: "
                f"{statistics.median(t['fused step']):.4f} ms against {sep:.4f} ms ({statistics.median(t['fused step']) - sep:+.4f} ms)")
            # ---- the orbit's wall time: 8 views, at most CAP iterations each in groups of 1; the target is what view 0 alone shows after 8 iterations
            CAP, VIEWS = 16, 8
            fresh = capi.Scene(path, res=(W, H))  # both rules see the same eight cameras: the scene's own and seven steps on
            cams = [fresh.camera] + [fresh.orbit(step, 0.0, 0.0) for _ in range(VIEWS - 1)]
            capi._check(L.pt_ctx_history_drop(ctx))
            capi._check(L.pt_ctx_set_camera(ctx, C.byref(cams[0])))
            capi._check(L.pt_ctx_render_until(ctx, 1, 8, 1, C.c_float(1000.0), C.byref(done), C.byref(psnr)))
            target = C.c_float(psnr.value)
            for rule in ("pt_render_until", "pt_history_render_until"):
                capi._check(L.pt_ctx_history_drop(ctx))
                capi._check(L.pt_ctx_sync(ctx))
                iters, t0 = [], time.perf_counter()
                for f in range(VIEWS):
                    capi._check(L.pt_ctx_set_camera(ctx, C.byref(cams[f])))
                    if rule == "pt_render_until":
                        capi._check(L.pt_ctx_render_until(ctx, f * CAP + 1, CAP, 1, target, C.byref(done), C.byref(psnr)))
                    else:
                        capi._check(L.pt_ctx_render_features(ctx, 1, 1))
                        if f:
                            capi._check(L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), VAR))
                        capi._check(L.pt_ctx_history_render_until(ctx, f * CAP + 1, CAP, 1, target, C.byref(done), C.byref(psnr), C.byref(view)))
                        capi._check(L.pt_ctx_history_capture_ex(ctx, C.c_float(done.value), VAR))
                    iters.append(done.value)
                capi._check(L.pt_ctx_sync(ctx))
                say(f"orbit of {VIEWS} views, target {target.value:.3f} dB, cap {CAP}, groups of 1, {rule:24s}: {1e3 * (time.perf_counter() - t0):9.2f} ms wall (moves, "
                    f"features, lookups and captures included), iterations per view {iters} = {sum(iters)}")

        if not name.startswith("cornell"):
            feedback_part()
            noise_part()
            continue
        capi._check(L.pt_ctx_history_drop(ctx))
        capi._check(L.pt_ctx_clear(ctx))
        capi._check(L.pt_ctx_render(ctx, 1, 1))
        capi._check(L.pt_ctx_render_features(ctx, 1, 1))

        def marked_share():
            """The share of pixels pt_history_denoise_ex's prepare marks at this view: rb > PT_HISTORY_MOMENTS_R_MAX, from the readbacks."""
            vc, c4 = np.empty((W * H, 4), np.float32), np.empty((W * H, 4), np.float32)
            capi._check(L.pt_ctx_readback_history_variance(ctx, None, capi._f(vc)))
            capi._check(L.pt_ctx_readback_history(ctx, None, capi._f(c4)))
            dn = np.float32(1) + c4[:, 3]
            wn, wh = np.float32(1) / dn, c4[:, 3] / dn
            rb = wn * wn + (wh * wh) * vc[:, 3]
            return float((~(rb <= capi.HISTORY_MOMENTS_R_MAX)).mean())

        t = timed([("denoise", lambda: L.pt_ctx_history_denoise_ex_device(ctx, one, None, MOM, C.byref(dev))),
                   ("capture", lambda: L.pt_ctx_history_capture_ex(ctx, one, MOM))])
        say("### with PT_HISTORY_MOMENTS, the first view (C absent): every pixel is marked for the spatial estimate")
        line("pt_history_denoise_ex (dev.)", t["denoise"])
        line("pt_history_capture_ex", t["capture"], 12 + 48 + 48 + 16)
        for f in range(1, 8):
            cam = scene.orbit(np.float32(2 * np.pi / 120), 0.0, 0.0)
            capi._check(L.pt_ctx_set_camera(ctx, C.byref(cam)))
            capi._check(L.pt_ctx_render(ctx, f + 1, 1))
            capi._check(L.pt_ctx_render_features(ctx, 1, 1))
            capi._check(L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), MOM))
            if f < 7:
                capi._check(L.pt_ctx_history_capture_ex(ctx, one, MOM))
        share = marked_share()
        t = timed([("reproject", lambda: L.pt_ctx_history_reproject_ex(ctx, C.byref(hopt), MOM)),
                   ("denoise", lambda: L.pt_ctx_history_denoise_ex_device(ctx, one, None, MOM, C.byref(dev))),
                   ("plain", lambda: L.pt_ctx_denoise_device(ctx, one, None, C.byref(dev)))])
        assert marked_share() == share  # no capture between the repetitions: every one looks the same history up and marks the same pixels
        t.update(timed([("capture", lambda: L.pt_ctx_history_capture_ex(ctx, one, MOM))]))  # (the same K and VK every time: C stays)
        say(f"### with PT_HISTORY_MOMENTS, a steady view (the 8th of an orbit, 1 iteration each): {100 * share:.3f} % of the pixels marked")
        line("pt_history_reproject_ex", t["reproject"], 48 + 16 + 16 + 4 * 64)
        line("pt_history_capture_ex", t["capture"], 12 + 48 + 16 + 48 + 16 + 16)
        line("pt_history_denoise_ex (dev.)", t["denoise"])
        line("pt_denoise (device)", t["plain"])
        say(f"the steady-view filter against pt_history_denoise above: {statistics.median(t['denoise']) - history_denoise_median:+.4f} ms "
            f"(one launch more, k_denoise_var_spatial, which leaves on a ballot in every wave without a marked pixel; no noise planes read)")
        feedback_part()
        noise_part()
    finally:
        L.pt_ctx_destroy(ctx)
out.close()
