"""The history round on the device (pt_history_round, pt_readback_history_extra, the counted forms of pt_history_resolve / _capture /
_capture_ex / _denoise_ex; csrc/pt_history.hip k_history_key, k_history_merge and the counted kernels, csrc/pt_denoise.hip
k_denoise_prepare_counted) against the library's host functions (the same bodies; pinned to the numpy restatement by
tests/test_history_round_host.py), bit for bit.  The host functions are always fed with the renderer's own readbacks, and the round's
samples are compared with the worker's own render of the same list (pt_stage_render_list_capacity), so these tests isolate the new code."""
import ctypes as C

import numpy as np
import pytest

import camera_scenes
import history_moments_ref as mref
import history_ref as href
import history_round_ref as ref
from history_ref import bits, f32

pytestmark = pytest.mark.gpu
RES = href.RES
W, H = RES
N = W * H
VAR, MOM = 1, 2  # PT_HISTORY_VARIANCE, PT_HISTORY_MOMENTS
SPP = 1
G = ref.SIM_GROUP


def same(got, want, what):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


@pytest.fixture(scope="module")
def orbit_paths(tmp_path_factory):
    return href.orbit_scene_paths(tmp_path_factory.mktemp("gpu_history_round"), camera_scenes.cornell_text)


def test_stage_equals_host(scene_dir):
    """The key kernel with the round's own selection, and the merge kernel, on the random planes of the host tests: one pixel, ragged
    last workgroups (185 = 37 x 5 pixels), exactly one workgroup (64 x 4), several (96 x 54); C absent and present; caps inside runs of
    equal keys; nothing fresh."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(32, 24)))
    try:
        for w, rows in ref.SHAPES:
            n = w * rows
            for seed, weights in ((0, (0.0, 1.0, 2.5, 4.0, 7.0, 32.0)), (1, (1.0, 2.0))):
                feat, Cp = ref.random_planes(w, rows, seed, weights)
                cases = [dict(current=None), dict(current=Cp), dict(current=Cp, min_history=2.5), dict(current=Cp, min_history=0.5)]
                fresh = capi.history_select_host(feat, w, rows, Cp, ref.EMITTER)[1]
                cases += [dict(current=Cp, max_fraction=max(c, 1) / n) for c in {1, fresh // 3, fresh // 2, fresh - 1, fresh} if c <= n]
                for kw in cases:
                    want, want_fresh, want_m = capi.history_select_host(feat, w, rows, emitter=ref.EMITTER, **kw)
                    got, got_fresh, got_m = capi.stage_history_select(feat, w, rows, emitter=ref.EMITTER, **kw)
                    assert (got_fresh, got_m) == (want_fresh, want_m), (w, rows, seed, kw)
                    assert np.array_equal(got, want), (w, rows, seed, kw)  # the entries behind m are -1 on both sides
            Cp[:, 3] = 4.0
            assert capi.stage_history_select(feat, w, rows, Cp, ref.EMITTER)[1:] == (0, 0)
            S, E = ref.random_image(n), ref.random_extra(n)
            rng = np.random.default_rng(n)
            for m in sorted({1, max(n // 3, 1), n}):
                lst = np.sort(rng.choice(n, m, replace=False)).astype(np.int32)
                Sw = ref.random_image(m, seed=3)
                want_S, want_E = capi.history_merge_host(S, E, lst, Sw, 4)
                got_S, got_E = capi.stage_history_merge(S, E, lst, Sw, 4)
                same(got_S, want_S, (w, rows, m, "S")), same(got_E, want_E, (w, rows, m, "E"))
    finally:
        r.free()


def view(capi, r, paths, f):
    """View f of the orbit up to the lookup: the camera, 1 spp, the feature pass, the lookup with moments."""
    cam = capi.Scene(paths[f], res=RES).camera
    if f > 0:
        r.set_camera(cam)
    r.render(f * SPP + 1, SPP)
    r.render_features(1, 1)
    if f > 0:
        r.history_reproject_ex(MOM)
    return cam


def current_planes(r, f):
    if f == 0:  # nothing captured yet: pt_readback_history refuses
        return None, None
    return r.readback_history()[1], r.readback_history_variance()[1]


@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
def test_renderer_sequence_equals_host(orbit_paths, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    emitter = capi.emitter_geoms(scene)
    assert emitter.any() and not emitter.all()
    r = capi.Renderer(scene, arith=arith)
    try:
        ms = []
        for f in range(3):
            view(capi, r, orbit_paths, f)
            Cp, VC = current_planes(r, f)
            S0, feat = r.readback(), r.readback_feature_planes()
            assert not r.readback_history_extra().any()  # a move cleared it
            samples0 = r.stats().samples
            first = 1000 + f * G + 1
            fresh, m = r.history_round(first, G)
            want_list, want_fresh, want_m = capi.history_select_host(feat, W, H, Cp, emitter)
            assert (fresh, m) == (want_fresh, want_m) and 0 < m < N, (f, fresh, m)
            want_list = want_list[:m]
            S1, E = r.readback(), r.readback_history_extra()
            assert np.array_equal(np.flatnonzero(E), want_list), f  # the list
            assert r.stats().samples - samples0 == G * m
            Sw = capi.stage_render_list_capacity(want_list, N, first, G)  # the round's worker (kept for cap = N pixels), the same list
            want_S, want_E = capi.history_merge_host(S0, np.zeros(N, f32), want_list, Sw, G)
            same(S1, want_S, (f, "S")), same(E, want_E, (f, "E"))
            rest = np.setdiff1d(np.arange(N), want_list)
            same(S1[rest], S0[rest], (f, "S elsewhere"))
            assert (E[want_list] == G).all() and Sw.any()
            same(r.history_resolve(SPP), capi.history_blend_counted_host(S1, SPP, E, Cp), (f, "pt_history_resolve"))
            same(r.history_denoise_ex(SPP), capi.history_denoise_moments_counted_host(S1, feat, W, H, SPP, E, Cp, VC), (f, "pt_history_denoise_ex"))
            r.history_capture_ex(SPP, MOM)
            K, VK = r.readback_history()[0], r.readback_history_variance()[0]
            same(K, capi.history_capture_counted_host(S1, feat, SPP, E, Cp), (f, "K"))
            same(VK, capi.history_capture_moments_counted_host(S1, SPP, E, Cp, VC), (f, "VK"))
            assert (K[0, want_list, 3] >= SPP + G).all()
            r.history_capture(SPP)  # the plain capture counts them too: the same K
            same(r.readback_history()[0], K, (f, "K of pt_history_capture"))
            r.history_capture_ex(SPP, MOM)
            ms.append(m)
        assert ms[1] < ms[0]  # the round limits itself
        if arith == "exact":
            assert ms == ref.SIM_ROUND_M[:3]
    finally:
        r.free()


def test_nothing_fresh_and_the_lifetime_of_the_extra_plane(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(orbit_paths[0], res=RES))
    try:
        view(capi, r, orbit_paths, 0)
        r.history_capture_ex(SPP, MOM)
        r.history_reproject_ex(MOM, keep_view_dependent=True)  # standing still, reflective geoms too: Th = 1 at every hit pixel
        S0, samples0 = r.readback(), r.stats().samples
        hit = r.readback_feature_planes()[1, :, 3] > 0
        assert (r.readback_history()[1][hit, 3] == 1).all()
        # min_history below every carried weight: nothing is fresh, nothing is rendered, E stays absent
        assert r.history_round(50, G, min_history=0.5) == (0, 0)
        before = r.stats().device_bytes  # (the selection's workspace, the worker and the emitter table exist now)
        same(r.readback(), S0, "nothing rendered"), same(r.readback_history_extra(), np.zeros(N, f32), "E absent")
        assert r.stats().samples == samples0
        assert r.history_round(50, G, min_history=0.5) == (0, 0) and r.stats().device_bytes == before
        r.noise_fold()  # E absent: nothing refuses
        before = r.stats().device_bytes  # (... and the fold's planes)
        # a round that renders: E appears, 4 bytes per pixel, once
        fresh, m = r.history_round(60, G, min_history=1.5)
        assert 0 < m == fresh < int(hit.sum())
        assert r.stats().device_bytes - before == 4 * N
        E = r.readback_history_extra()
        assert int((E == G).sum()) == m and int((E == 0).sum()) == N - m
        grown = r.stats().device_bytes
        r.history_round(70, G, min_history=1.5)  # the same pixels again: Th has not changed
        same(r.readback_history_extra(), E + E, "E after a second round")
        assert r.stats().device_bytes == grown
        r.history_drop()  # E belongs to S, not to K
        same(r.readback_history_extra(), E + E, "E after pt_history_drop")
        with pytest.raises(capi.PtError, match="pt_noise_fold"):
            r.noise_fold()
        r.clear()
        assert not r.readback_history_extra().any()
        r.render(1, 1)
        r.noise_fold()  # absent again: nothing refuses
        r.render_features(1, 1)
        fresh, m = r.history_round(80, G)  # C absent (the clear): every non-emitter hit pixel
        E = r.readback_history_extra()
        assert m == fresh > 0 and int((E == G).sum()) == m and int((E == 0).sum()) == N - m  # zeroed by the clear, not added to
        r.set_camera(capi.Scene(orbit_paths[1], res=RES).camera)
        assert not r.readback_history_extra().any()
        r.render(2, 1)
        r.noise_fold()
    finally:
        r.free()


def test_the_orbit_of_the_simulation_on_the_device(orbit_paths):
    """The exact build reproduces the oracle's samples bit for bit, so the orbit of tests/test_history_round_sim.py run on the renderer
    gives the simulation's figures; the 1024-spp frame at the last camera comes from the renderer too."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(orbit_paths[0], res=RES), arith="exact")
    try:
        ms = []
        for f in range(href.FRAMES):
            view(capi, r, orbit_paths, f)
            ms.append(r.history_round(1000 + f * G + 1, G)[1])
            blend, filtered = r.history_resolve(SPP), r.history_denoise_ex(SPP)
            r.history_capture_ex(SPP, MOM)
    finally:
        r.free()
    r = capi.Renderer(capi.Scene(orbit_paths[-1], res=RES), arith="exact")
    try:
        r.render(href.TRUTH_FIRST, href.TRUTH_SPP)
        truth = r.readback().astype(np.float64) / href.TRUTH_SPP
    finally:
        r.free()
    carried, both = href.mse(blend, truth), href.mse(filtered, truth)
    samples = (href.FRAMES * N + G * sum(ms)) / (href.FRAMES * N)
    print(f"orbit at 1 spp with rounds of {G} on the device, last view: MSE blend {carried:.9g}, filtered blend {both:.9g}, samples {samples:.9g} x, m {ms}")
    assert ms == ref.SIM_ROUND_M
    assert carried < mref.SIM_BLEND and both < mref.SIM_FILTERED
    for got, pinned in ((carried, ref.SIM_ROUND_BLEND), (both, ref.SIM_ROUND_FILTERED), (samples, ref.SIM_ROUND_SAMPLES)):
        assert abs(got / pinned - 1) < 1e-6, (got, pinned)


def test_refusals_by_name_and_order(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    L = capi.lib()

    def refused(rc, *phrases):
        assert rc != 0
        msg = L.pt_last_error().decode()
        for ph in phrases:
            assert ph in msg, (ph, msg)

    def opts(min_history=0.0, max_fraction=0.0):
        return C.byref(capi.PtHistoryRoundOptions(min_history, max_fraction))

    who = "pt_history_round"
    capi.pt_free()
    refused(L.pt_history_round(0, 0, opts(-1.0), None, None), who, "pt_init")
    refused(L.pt_readback_history_extra(None), "pt_readback_history_extra", "pt_init")
    # the iterations, then the convergence metric, then the ragged tile
    r = capi.Renderer(scene, pixel_begin=10, pixel_count=W * 3, convergence=2)
    try:
        before = r.stats().device_bytes
        refused(L.pt_history_round(0, 1, opts(-1.0), None, None), who, "iterations 0")
        refused(L.pt_history_round(1, 0, opts(-1.0), None, None), who, "iterations 1, +0")
        refused(L.pt_history_round(2 ** 31 - 2, 3, opts(-1.0), None, None), who, "iterations")
        refused(L.pt_history_round(1, 1, opts(-1.0), None, None), who, "convergence")
        assert r.stats().device_bytes == before
    finally:
        r.free()
    r = capi.Renderer(scene, pixel_begin=10, pixel_count=W * 3)
    try:
        before = r.stats().device_bytes
        refused(L.pt_history_round(0, 1, opts(-1.0), None, None), who, "iterations 0")
        refused(L.pt_history_round(1, 1, opts(-1.0), None, None), who, "whole contiguous image rows")
        assert r.stats().device_bytes == before
    finally:
        r.free()
    r = capi.Renderer(scene)
    try:
        before = r.stats().device_bytes
        refused(L.pt_history_round(1, 1, opts(-1.0), None, None), who, "no feature pass")
        refused(L.pt_readback_history_extra(None), "pt_readback_history_extra", "null")
        assert r.stats().device_bytes == before
        r.render(1, 1)
        r.render_features(1, 1)
        before = r.stats().device_bytes
        for bad, phrase in ((opts(float("nan")), "finite"), (opts(float("inf")), "finite"), (opts(0.0, float("nan")), "finite"), (opts(-1.0), "min_history"),
                            (opts(0.0, -0.25), "max_fraction"), (opts(0.0, 1.5), "max_fraction")):
            refused(L.pt_history_round(1, 1, bad, None, None), who, phrase)
        assert r.stats().device_bytes == before  # nothing allocated by any of them
        assert not r.readback_history_extra().any()
        # the adaptive state comes before the feature pass
        r.clear()
        for g in range(2):
            r.render(g * 4 + 1, 4)
            r.noise_fold()
        r.adaptive_round(9, 4, 0.25)
        refused(L.pt_history_round(1, 1, opts(-1.0), None, None), who, "adaptive state")
    finally:
        r.free()


def test_what_reads_a_uniform_sum_refuses_while_extras_are_present(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(orbit_paths[0], res=RES))
    try:
        for g in range(2):
            r.render(g + 1, 1)
            r.noise_fold()
        r.render_features(1, 1)
        r.denoise_guided(), r.resolve(), r.save_u8(2)  # all fine before the round
        fresh, m = r.history_round(100, G)
        assert m > 0
        before = r.stats().device_bytes
        calls = {
            "pt_noise_fold": r.noise_fold,
            "pt_render_until": lambda: r.render_until(200, 4, 30.0, 2),
            "pt_denoise": lambda: r.denoise(2),
            "pt_denoise_guided": r.denoise_guided,
            "pt_denoise_adaptive": r.denoise_adaptive,
            "pt_history_denoise": lambda: r.history_denoise(2),
            "pt_history_denoise_ex": lambda: r.history_denoise_ex(2, 0),
            "pt_history_capture_ex": lambda: r.history_capture_ex(2, VAR),
            "pt_adaptive_round": lambda: r.adaptive_round(200, 2, 0.25),
            "pt_adaptive_round_threshold": lambda: r.adaptive_round_threshold(200, 2, 0.01, 0.25),
            "pt_adaptive_round_list": lambda: r.adaptive_round_list(200, 2, np.arange(4, dtype=np.int32), 4),
            "pt_render_adaptive": lambda: r.render_adaptive(200, 4, 30.0, 0.25, 2),
            "pt_render_threshold": lambda: r.render_threshold(200, 4, 0.01, 0.25, 2),
            "pt_resolve": r.resolve,
            "pt_save_u8": lambda: r.save_u8(2),
            "pt_preview_rgba8": lambda: r.preview(2),
        }
        for name, call in calls.items():
            with pytest.raises(capi.PtError) as e:
                call()
            msg = str(e.value)
            assert msg.startswith(name + ":") and "pt_history_resolve" in msg and "pt_clear" in msg, (name, msg)
        assert r.stats().device_bytes == before  # nothing allocated by any of them
        # these keep working
        r.render(3, 1)
        r.render_features(1, 1)
        r.readback(), r.stats()
        r.history_capture_ex(3, MOM)
        r.history_reproject_ex(MOM)
        r.history_reproject()
        r.history_resolve(3)
        r.history_capture(3)
        r.clear()
        r.render(1, 1)
        r.noise_fold()  # back in the uniform state
    finally:
        r.free()
