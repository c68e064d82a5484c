"""Threshold rounds over the blend on the device (pt_history_round_threshold, pt_history_render_threshold, pt_history_noise_adaptive,
pt_history_resolve_adaptive, pt_history_capture_adaptive, pt_history_denoise_adaptive; csrc/pt_history_threshold.hip and the
HistoryAdaptive prepare of csrc/pt_denoise.hip) against the library's host twins (the same bodies; pinned to the numpy restatement by
tests/test_history_threshold_host.py), bit for bit.  The host twins are always fed with the renderer's own readbacks, so these tests
isolate the new code."""
import ctypes as C
import struct

import numpy as np
import pytest

import camera_scenes
import denoise_ref
import history_ref as href
import history_threshold_ref as ref
from history_ref import bits, f32

pytestmark = pytest.mark.gpu
RES = href.RES
W, H = RES
N = W * H
G = 2  # iterations per group and per round
ARITHS = ["exact", "fma", "fast"]


def same(got, want, what):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


def dbits(x):
    return struct.pack("<d", x)


def state_bytes(n):
    return 4 * n + 8 * ((n + 1023) // 1024 + 1)


@pytest.fixture(scope="module")
def orbit_paths(tmp_path_factory):
    return href.orbit_scene_paths(tmp_path_factory.mktemp("gpu_history_threshold"), camera_scenes.cornell_text)


def raw_planes(r, capi):
    out = np.empty((2, r.n, 4), f32)
    capi._check(capi.lib().pt_readback_noise(capi._f(out)))
    return out


def state(r, capi):
    """The SUM image, the noise planes and the counts as they lie."""
    return r.readback(), raw_planes(r, capi), r.readback_adaptive()


def uniform_groups(r, first, groups=2):
    for g in range(groups):
        r.render(first + g * G, G)
        r.noise_fold()


def first_view(r):
    """View 0: two groups with a fold after each, the features, the capture with variance."""
    uniform_groups(r, 1)
    r.render_features(1, 1)
    r.history_capture_ex(2 * G)


def move(r, capi, path):
    """The move to the camera of `path` and the lookup with variance: C and VC present, nothing rendered yet."""
    r.set_camera(capi.Scene(path, res=RES).camera)
    r.render_features(1, 1)
    r.history_reproject_ex()


def current(r):
    return r.readback_history()[1], r.readback_history_variance()[1]


def threshold_for(planes, counts, Cp, VC, rank):
    """A threshold that leaves about `rank` pixels above: just above the square root of the blend's key at that rank."""
    w, ne, _, _ = ref.noise_counts(planes, counts, Cp, VC)
    k = np.sort(ref.keys_blend(w, ne, W, H).view(f32))[::-1]
    return float(np.sqrt(np.float64(k[rank]))) * (1 + 1e-6)


# ---- 1. the stage entries against the host twins ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=[f"{w}x{r}" for w, r in ref.SHAPES])
def test_stage_entries_equal_host_twins(scene_dir, shape, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, rows = shape
    n = w * rows
    counts = ref.random_counts(n)
    noise, S = ref.noise_planes(counts)
    _, feat = denoise_ref.random_frame(w, rows, 4)
    Cp, VC = ref.current_planes(n, 3 * n)
    tame = np.where(np.isfinite(VC) & (VC < f32(1e30)), VC, f32(2.0)).astype(f32)
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(32, 24)), arith=arith)
    try:
        for cur, var, what in ((None, None, "absent"), (Cp, VC, "present")):
            wp, ne, sse = capi.stage_history_noise_adaptive(noise, counts, cur, var)
            want_w, want_ne, want_vb, want_sse = capi.history_noise_adaptive_host(noise, counts, cur, var)
            same(wp, want_w, (shape, what, "W")), same(ne, want_ne, (shape, what, "NE"))
            finite = np.isfinite(want_w)
            exact = float(np.sum(want_w[finite].astype(np.float64)))
            assert np.isnan(sse) == np.isnan(want_sse) and (np.isnan(sse) or np.isinf(sse) or abs(sse - exact) <= 1e-9 * abs(exact)), (shape, what, sse, want_sse)
            assert dbits(capi.stage_history_noise_adaptive(noise, counts, cur, var)[2]) == dbits(sse)  # no atomics: equal inputs, equal bits
            for name, thr in ref.thresholds(noise, counts, w, rows, cur, var).items():
                for cap in ref.caps(n):
                    got = capi.stage_history_select_threshold_blend(noise, counts, w, rows, thr, cap, cur, var)
                    want = capi.history_select_threshold_blend_host(noise, counts, w, rows, thr, cap, cur, var)
                    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (shape, what, name, cap, got[1:], want[1:])
            K, VK, avg = capi.stage_history_capture_adaptive(S, feat, noise, counts, cur, var)
            want_K, want_VK = capi.history_capture_adaptive_host(S, feat, noise, counts, cur, var)
            same(K, want_K, (shape, what, "K")), same(VK, want_VK, (shape, what, "VK")), same(VK, want_vb, (shape, what, "VK is vb"))
            same(avg, capi.history_blend_adaptive_host(S, counts, cur), (shape, what, "blend"))
            fv = None if var is None else tame
            same(capi.stage_history_denoise_adaptive(S, feat, noise, counts, w, rows, cur, fv, levels=2),
                 capi.history_denoise_adaptive_host(S, feat, noise, counts, w, rows, cur, fv, levels=2), (shape, what, "filter"))
        tn, tc, tC, tVC, thr = ref.tie_planes(w, rows)  # keys exactly equal to thr are not above
        got = capi.stage_history_select_threshold_blend(tn, tc, w, rows, thr, n, tC, tVC)
        want = capi.history_select_threshold_blend_host(tn, tc, w, rows, thr, n, tC, tVC)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:] and want[1] < n
    finally:
        r.free()


# ---- 2. a live renderer: rounds, driver and what follows ----------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
def test_rounds_driver_and_follow_on_equal_host_twins(orbit_paths, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    cap_iters, first = 16, 101
    # (one renderer at a time.)  The second renderer of the issue first: the uniform groups, then pt_adaptive_round_list over the list the
    # host twin selects from its readbacks — which the first renderer's must equal round by round, so they are the same readbacks
    b = capi.Renderer(scene, arith=arith)
    try:
        first_view(b)
        move(b, capi, orbit_paths[1])
        Cp, VC = current(b)
        assert (Cp[:, 3] > 0).any() and (Cp[:, 3] == 0).any() and (VC[:, :3] > 0).any()
        uniform_groups(b, first)
        S, planes, counts = state(b, capi)
        E = threshold_for(planes, counts, Cp, VC, N // 4)
        plain_above = capi.adaptive_select_threshold_host(planes, counts, W, H, E, N)[1]
        lists, states, used, samples = [], [], 2 * G, 2 * G * N
        while used < cap_iters:
            S, planes, counts = state(b, capi)
            lst, above, m = capi.history_select_threshold_blend_host(planes, counts, W, H, E, N, Cp, VC)
            lists.append((lst, above, m))
            if above <= 0:
                break
            b.adaptive_round_list(first + used, G, lst, N)
            used += G
            samples += G * m
            states.append(state(b, capi))
        assert len(states) >= 2 and lists[0][1] < plain_above  # the history takes pixels off the list
        assert lists[1][2] < lists[0][2]
        final = state(b, capi)
        feat = b.readback_feature_planes()
    finally:
        b.free()
    a = capi.Renderer(scene, arith=arith)
    try:
        first_view(a)
        move(a, capi, orbit_paths[1])
        uniform_groups(a, first)
        done = 2 * G
        same(current(a)[0], Cp, "C"), same(current(a)[1], VC, "VC")
        for k, (lst, above, m) in enumerate(lists):
            got = a.history_round_threshold(first + done, G, E, 1.0)
            assert got == (above, m), (arith, k, got, above, m)
            if above <= 0:
                break
            done += G
            for x, y, name in zip(state(a, capi), states[k], ("S", "planes", "counts")):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (arith, k, name)
            with pytest.raises(capi.PtError, match="pt_readback_history_noise: no estimate"):
                a.readback_history_noise()  # a round that rendered: the image W described is gone
        assert a.stats().samples == samples
        # what follows the rounds: estimate, resolve, filter, capture, and the next view's lookup
        S, planes, counts = final
        sse = a.history_noise_adaptive()
        want_w, want_ne, want_vb, want_sse = capi.history_noise_adaptive_host(planes, counts, Cp, VC)
        same(a.readback_history_noise(), want_w, "W"), same(a.readback_history_noise_samples(), want_ne, "NE")
        assert abs(sse - want_sse) <= 1e-9 * want_sse
        same(a.history_resolve_adaptive(), capi.history_blend_adaptive_host(S, counts, Cp), "resolve")
        same(a.history_denoise_adaptive(levels=3), capi.history_denoise_adaptive_host(S, feat, planes, counts, W, H, Cp, VC, levels=3), "filter")
        a.history_capture_adaptive()
        K, VK = a.readback_history()[0], a.readback_history_variance()[0]
        want_K, want_VK = capi.history_capture_adaptive_host(S, feat, planes, counts, Cp, VC)
        same(K, want_K, "K"), same(VK, want_VK, "VK")
        kept_cam = capi.Scene(orbit_paths[1], res=RES).camera
        move(a, capi, orbit_paths[2])
        assert (a.readback_adaptive() == 0).all()  # the move left the adaptive state as pt_clear does
        C2, VC2 = current(a)
        want_C2, want_VC2 = capi.history_reproject_variance_host(kept_cam, K, a.readback_feature_planes(), capi.reject_geoms(scene), VK, W, H)
        same(C2, want_C2, "the next view's C"), same(VC2, want_VC2, "the next view's VC")
        assert (C2[:, 3] > 2 * G).any()  # weights beyond one view's uniform samples travelled on
    finally:
        a.free()
    # the driver: the same groups and rounds in one call
    d = capi.Renderer(scene, arith=arith)
    try:
        first_view(d)
        move(d, capi, orbit_paths[1])
        got = d.history_render_threshold(first, cap_iters, E, 1.0, G, 0)
        assert got == (used, samples, lists[-1][1]), (got, used, samples, lists[-1][1])
        for x, y, name in zip(state(d, capi), final, ("S", "planes", "counts")):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (arith, "driver", name)
        assert d.stats().samples == samples
    finally:
        d.free()


# ---- 3. without history the calls are the adaptive ones -------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
def test_without_history_the_calls_are_the_adaptive_ones(orbit_paths, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    got = []
    for blend in (True, False):
        r = capi.Renderer(scene, arith=arith)
        try:
            uniform_groups(r, 1)
            r.render_features(1, 1)
            S, planes, counts = state(r, capi)
            E = threshold_for(planes, counts, None, None, N // 3)
            one = (r.history_round_threshold if blend else r.adaptive_round_threshold)(2 * G + 1, G, E, 0.25)
            after_round = state(r, capi)
            resolved = r.history_resolve_adaptive() if blend else r.resolve()
            filtered = r.history_denoise_adaptive(levels=2) if blend else r.denoise_adaptive(levels=2)
            r.clear()
            run = (r.history_render_threshold if blend else r.render_threshold)(1, 16, E, 0.25, G, 5)
            got.append((one, after_round, resolved, filtered, run, state(r, capi), r.stats().samples))
        finally:
            r.free()
    (one0, st0, res0, fil0, run0, end0, n0), (one1, st1, res1, fil1, run1, end1, n1) = got
    assert one0 == one1 and one0[1] > 0 and run0 == run1 and n0 == n1, (one0, one1, run0, run1)
    for x, y, name in zip(st0 + end0, st1 + end1, ("S", "planes", "counts") * 2):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (arith, name)
    same(res0, res1, "pt_history_resolve_adaptive is pt_resolve"), same(fil0, fil1, "pt_history_denoise_adaptive is pt_denoise_adaptive")


# ---- 4. the uniform state with C present ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
def test_in_the_uniform_state_the_calls_are_the_history_ones(orbit_paths, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    T = 2 * G
    got = []
    for counted in (True, False):
        r = capi.Renderer(scene, arith=arith)
        try:
            first_view(r)
            move(r, capi, orbit_paths[1])
            uniform_groups(r, 50)
            resolved = r.history_resolve_adaptive() if counted else r.history_resolve(T)
            sse = r.history_noise_adaptive() if counted else r.history_noise(T)
            w = r.readback_history_noise()
            if counted:
                same(r.readback_history_noise_samples(), (f32(T) + current(r)[0][:, 3]).astype(f32), "NE")
                r.history_capture_adaptive()
            else:
                r.history_capture_ex(T)
            got.append((resolved, dbits(sse), w, r.readback_history()[0], r.readback_history_variance()[0]))
        finally:
            r.free()
    assert got[0][1] == got[1][1]
    for x, y, name in zip(got[0], got[1], ("resolve", None, "W", "K", "VK")):
        if name:
            same(x, y, (arith, name))


# ---- 5. refusals and memory --------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_phrase_and_order_and_memory(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    L = capi.lib()
    out = np.empty((N, 3), f32)
    fp = capi._f(out)

    def refused(rc, *phrases):
        assert rc != 0
        msg = L.pt_last_error().decode()
        for ph in phrases:
            assert ph in msg, (ph, msg)

    def round_(first=5, group=G, thr=0.1, frac=1.0):
        return L.pt_history_round_threshold(first, group, C.c_float(thr), C.c_float(frac), None, None)

    def driver(first=5, count=4, group=G, thr=0.1, frac=1.0, min_pixels=0):
        return L.pt_history_render_threshold(first, count, group, C.c_float(thr), C.c_float(frac), min_pixels, None, None, None)

    steps = {"pt_history_noise_adaptive": lambda: L.pt_history_noise_adaptive(None), "pt_history_resolve_adaptive": lambda: L.pt_history_resolve_adaptive(fp),
             "pt_history_capture_adaptive": lambda: L.pt_history_capture_adaptive(), "pt_history_denoise_adaptive": lambda: L.pt_history_denoise_adaptive(None, fp)}
    capi.pt_free()
    for who, call in dict(steps, pt_history_round_threshold=round_, pt_history_render_threshold=driver).items():
        refused(call(), who, "pt_init")
    r = capi.Renderer(scene, pixel_begin=10, pixel_count=W * 3)  # a ragged tile
    try:
        before = r.stats().device_bytes
        for who, call in dict(steps, pt_history_round_threshold=round_, pt_history_render_threshold=driver).items():
            refused(call(), who, "whole contiguous image rows")
        assert r.stats().device_bytes == before
    finally:
        r.free()
    r = capi.Renderer(scene)
    try:
        before = r.stats().device_bytes
        # what pt_adaptive_round_threshold and pt_render_threshold refuse, in their order and words, under the new names
        for new, old, args in ((round_, lambda **kw: L.pt_adaptive_round_threshold(kw.get("first", 5), kw.get("group", G), C.c_float(kw.get("thr", 0.1)),
                                                                                    C.c_float(kw.get("frac", 1.0)), None, None), "pt_adaptive_round_threshold"),
                               (driver, lambda **kw: L.pt_render_threshold(kw.get("first", 5), kw.get("count", 4), kw.get("group", G), C.c_float(kw.get("thr", 0.1)),
                                                                           C.c_float(kw.get("frac", 1.0)), kw.get("min_pixels", 0), None, None, None),
                                "pt_render_threshold")):
            name = "pt_history_round_threshold" if new is round_ else "pt_history_render_threshold"
            cases = [dict(first=0), dict(frac=0.0), dict(frac=1.5), dict(thr=-1.0), dict(thr=float("nan"))]
            cases += [dict(group=0), dict()] if new is round_ else [dict(count=0), dict(group=-1), dict(min_pixels=-1)]
            for kw in cases:
                refused(new(**kw), name + ":")
                msg = L.pt_last_error().decode()
                assert old(**kw) != 0 and L.pt_last_error().decode().replace(args, name) == msg, (kw, msg)
        assert r.stats().device_bytes == before
        for who, call in steps.items():
            if who == "pt_history_capture_adaptive" or who == "pt_history_denoise_adaptive":
                refused(call(), who, "no feature pass")
            else:
                refused(call(), who, "nothing has been folded")
        r.render_features(1, 1)
        before = r.stats().device_bytes
        for who, call in steps.items():
            refused(call(), who, "nothing has been folded")
        refused(L.pt_history_denoise_adaptive(C.byref(capi.denoise_options(levels=9)), fp), "pt_history_denoise_adaptive", "levels")  # the options before the folds
        r.render(1, G)
        r.noise_fold()
        before = r.stats().device_bytes  # (the fold's planes)
        for who, call in steps.items():
            refused(call(), who, "1 group(s) folded")
        refused(round_(), "pt_history_round_threshold", "1 group(s) folded")
        r.render(1 + G, G)
        for who, call in steps.items():
            refused(call(), who, "1 group(s) folded")
        r.noise_fold()
        r.render(1 + 2 * G, 1)
        for who, call in steps.items():
            refused(call(), who, "fold first")
        refused(round_(), "pt_history_round_threshold", "fold first")
        r.noise_fold()
        refused(L.pt_history_resolve_adaptive(None), "pt_history_resolve_adaptive", "null")
        refused(L.pt_history_denoise_adaptive(None, None), "pt_history_denoise_adaptive", "null")
        refused(L.pt_readback_history_noise_samples(fp), "pt_readback_history_noise_samples", "no estimate")
        assert r.stats().device_bytes == before  # nothing allocated by any of them
        # C present with VC absent, or of the moments kind: the last refusal of every call
        r.history_capture(2 * G + 1)
        r.history_reproject()
        before = r.stats().device_bytes
        for who, call in dict(steps, pt_history_round_threshold=round_, pt_history_render_threshold=driver).items():
            refused(call(), who, "the current plane has no variance", "PT_HISTORY_VARIANCE")
        refused(round_(thr=-1.0), "pt_history_round_threshold", "threshold")  # the adaptive rounds' refusals come first
        r.clear()
        uniform_groups(r, 1)
        r.render_features(1, 1)
        r.history_capture_ex(2 * G, 2)
        r.history_reproject_ex(2)
        before = r.stats().device_bytes
        for who, call in dict(steps, pt_history_round_threshold=round_, pt_history_render_threshold=driver).items():
            refused(call(), who, "the current plane has no variance")
        assert r.stats().device_bytes == before and r.noise()["iterations"] == 2 * G  # nothing was rendered by the refused rounds
        # the extra plane: the message of the other uniform-sum readers
        r.clear()
        r.render(1, 1)
        r.render_features(1, 1)
        fresh, selected = r.history_round(2, 1)
        assert selected > 0
        before = r.stats().device_bytes
        for who, call in dict(steps, pt_history_round_threshold=round_, pt_history_render_threshold=driver).items():
            refused(call(), who, "extra samples", "pt_clear")
        assert r.stats().device_bytes == before
        # every history call the library had still refuses the adaptive state; the new ones run in it
        r.clear()
        uniform_groups(r, 1)
        r.render_features(1, 1)
        r.history_capture_ex(2 * G)
        bytes_old_calls = r.stats().device_bytes
        r.history_noise(2 * G)
        assert r.stats().device_bytes == bytes_old_calls + state_bytes(N)  # as before: W and the partial sums, no NE
        r.history_noise_adaptive()
        assert r.stats().device_bytes == bytes_old_calls + state_bytes(N) + 4 * N  # NE: the first call that needs it
        above, selected = r.history_round_threshold(2 * G + 1, G, 0.0, 0.25)
        assert selected > 0
        in_round = r.stats().device_bytes
        d = C.c_double(0.0)
        old = {"pt_history_capture": lambda: L.pt_history_capture(C.c_float(4.0)), "pt_history_capture_ex": lambda: L.pt_history_capture_ex(C.c_float(4.0), 1),
               "pt_history_reproject": lambda: L.pt_history_reproject(None), "pt_history_reproject_ex": lambda: L.pt_history_reproject_ex(None, 1),
               "pt_history_resolve": lambda: L.pt_history_resolve(C.c_float(4.0), fp), "pt_history_denoise": lambda: L.pt_history_denoise(C.c_float(4.0), None, fp),
               "pt_history_denoise_ex": lambda: L.pt_history_denoise_ex(C.c_float(4.0), None, 2, fp), "pt_history_noise": lambda: L.pt_history_noise(C.c_float(4.0), 1, C.byref(d)),
               "pt_history_render_until": lambda: L.pt_history_render_until(9, 2, 1, C.c_float(30.0), None, None, None),
               "pt_history_round": lambda: L.pt_history_round(9, 1, None, None, None)}
        for who, call in old.items():
            refused(call(), who, "adaptive state")
        for who, call in steps.items():
            assert call() == 0, (who, L.pt_last_error().decode())
        assert r.stats().device_bytes >= in_round
    finally:
        r.free()


# ---- 6. the orbit of the simulation ----------------------------------------------------------------------------------------------------------
def test_the_orbit_of_the_simulation_on_the_device(orbit_paths):
    """The exact build reproduces the oracle's samples bit for bit and the keys are the host twins', so the orbit of
    tests/test_history_threshold_sim.py on the renderer takes the simulation's iteration numbers and samples per view under both rules, and
    ends with its errors."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    cap, group, min_pixels = ref.ORBIT_CAP, ref.ORBIT_GROUP, ref.ORBIT_MIN_PIXELS
    r = capi.Renderer(capi.Scene(orbit_paths[0], res=RES), arith="exact")
    try:
        alone, blend = [], []
        for f in range(href.FRAMES):
            if f > 0:
                r.set_camera(capi.Scene(orbit_paths[f], res=RES).camera)
            alone.append(r.render_threshold(f * cap + 1, cap, ref.SIM_E, ref.ORBIT_FRACTION, group, min_pixels)[:2])
            r.clear()
            r.render_features(1, 1)
            if f > 0:
                r.history_reproject_ex()
            blend.append(r.history_render_threshold(f * cap + 1, cap, ref.SIM_E, ref.ORBIT_FRACTION, group, min_pixels)[:2])
            if f == href.FRAMES - 1:
                resolved, filtered = r.history_resolve_adaptive(), r.history_denoise_adaptive()
            r.history_capture_adaptive()
        print(f"E {ref.SIM_E}: (iteration numbers, samples) per view alone {alone}, with the blend's key {blend}")
        assert tuple(a[0] for a in alone) == ref.SIM_ALONE_USED and tuple(a[1] for a in alone) == ref.SIM_ALONE_SAMPLES
        assert tuple(b[0] for b in blend) == ref.SIM_BLEND_USED and tuple(b[1] for b in blend) == ref.SIM_BLEND_SAMPLES
        r.clear()
        r.render(href.TRUTH_FIRST, href.TRUTH_SPP)
        truth = r.readback().astype(np.float64) / href.TRUTH_SPP
        mse = float(((resolved.astype(np.float64) - truth) ** 2).sum() / (3 * N))
        mse_filtered = float(((filtered.astype(np.float64) - truth) ** 2).sum() / (3 * N))
        print(f"the last view: MSE of the blend {mse:.6e}, filtered {mse_filtered:.6e}")
        assert abs(mse / ref.SIM_LAST_MSE - 1) < 1e-5 and abs(mse_filtered / ref.SIM_LAST_MSE_FILTERED - 1) < 1e-5
    finally:
        r.free()
