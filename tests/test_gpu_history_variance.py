"""The variance of the history and the filter over the blend on the device (pt_history_capture_ex / _reproject_ex with
PT_HISTORY_VARIANCE, pt_history_denoise; csrc/pt_history.hip, csrc/pt_denoise.hip) against the library's host functions (the same
bodies; pinned to the numpy restatement by tests/test_history_variance_host.py), bit for bit.  The host functions are always fed with
the renderer's own readbacks, so these tests isolate the new code."""
import ctypes as C

import numpy as np
import pytest

import camera_scenes
import denoise_guided_ref
import denoise_ref
import history_ref as href
import history_variance_ref as ref
from history_ref import bits, f32

pytestmark = pytest.mark.gpu
RES, SPP, GROUPS = href.RES, href.SPP, ref.GROUPS
W, H = RES
VAR = 1  # PT_HISTORY_VARIANCE


def same(got, want, what):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


@pytest.fixture(scope="module")
def orbit_paths(tmp_path_factory):
    return href.orbit_scene_paths(tmp_path_factory.mktemp("gpu_history_variance"), camera_scenes.cornell_text)


class Default:
    """The default instance (capi.Renderer) behind the names the sequence below calls."""

    def __init__(self, scene, **kw):
        from cosc_4397_pathtracing_raytracing_project_amd import capi
        self.capi, self.r, self.n, self.row0, self.rows = capi, capi.Renderer(scene, **kw), W * H, 0, H

    def call(self, name, *args):
        self.capi._check(getattr(self.capi.lib(), "pt_" + name)(*args))

    def free(self):
        self.r.free()


class Context:
    """A context of one's own (pt_ctx_*) over frame rows row0 .. row0 + rows - 1."""

    def __init__(self, scene, row0, rows, **kw):
        from cosc_4397_pathtracing_raytracing_project_amd import capi
        self.capi, self.n, self.row0, self.rows = capi, W * rows, row0, rows
        self.h = C.c_void_p()
        opt = capi.make_options(pixel_begin=row0 * W, pixel_count=W * rows, **kw)
        capi._check(capi.lib().pt_ctx_create(C.byref(scene.desc), C.byref(opt), C.byref(self.h)))

    def call(self, name, *args):
        self.capi._check(getattr(self.capi.lib(), "pt_ctx_" + name)(self.h, *args))

    def free(self):
        self.capi.lib().pt_ctx_destroy(self.h)


def out(api, *shape):
    a = np.empty(shape, f32)
    return a, api.capi._f(a)


def view_readbacks(api):
    """(S, feature planes, noise planes) of the tile as they lie."""
    S, ps = out(api, api.n, 3)
    feat, pf = out(api, 3, api.n, 4)
    noise, pn = out(api, 2, api.n, 4)
    api.call("readback", ps), api.call("readback_features", pf), api.call("readback_noise", pn)
    return S, feat, noise


def history_readbacks(api):
    K, pk = out(api, 3, api.n, 4)
    Cp, pc = out(api, api.n, 4)
    VK, pvk = out(api, api.n, 4)
    VC, pvc = out(api, api.n, 4)
    api.call("readback_history", pk, pc), api.call("readback_history_variance", pvk, pvc)
    return K, Cp, VK, VC


def sequence(api, paths, views, device_tables_at=2):
    """The command line's --denoise-history order through `views` views: per view what the renderer read back (camera, S, features,
    noise) and what it made of them (C, VC, blend, filtered blend, K, VK)."""
    capi = api.capi
    seen, made = [], []
    for f in range(views):
        cam = capi.Scene(paths[f], res=RES).camera
        if f > 0:
            if f == device_tables_at:
                api.call("set_camera_ex", C.byref(cam), capi.PT_SET_CAMERA_DEVICE_TABLES)
            else:
                api.call("set_camera", C.byref(cam))
        for g in range(GROUPS):
            api.call("render", f * SPP + g * (SPP // GROUPS) + 1, SPP // GROUPS)
            api.call("noise_fold")
        api.call("render_features", 1, 1)
        if f > 0:
            api.call("history_reproject_ex", None, VAR)
        blend, pb = out(api, api.n, 3)
        filtered, pf = out(api, api.n, 3)
        api.call("history_resolve", C.c_float(SPP), pb)
        api.call("history_denoise", C.c_float(SPP), None, pf)
        if f > 0:
            _, Cp, _, VC = history_readbacks(api)
        else:  # nothing captured yet: pt_readback_history refuses, the variance's readback gives zeros
            Cp, (VC, pv) = np.zeros((api.n, 4), f32), out(api, api.n, 4)
            api.call("readback_history_variance", None, pv)
        seen.append((cam,) + view_readbacks(api))
        api.call("history_capture_ex", C.c_float(SPP), VAR)
        K, _, VK, _ = history_readbacks(api)
        made.append((Cp, VC, blend, filtered, K, VK))
    return seen, made


def check_against_host(api, scene, seen, made, what):
    capi = api.capi
    reject = capi.reject_geoms(scene)
    K = VK = kept_cam = None
    for f, ((cam, S, feat, noise), (C_dev, VC_dev, blend, filtered, K_dev, VK_dev)) in enumerate(zip(seen, made)):
        Cp = VC = None
        if K is not None:
            Cp, VC = capi.history_reproject_variance_host(kept_cam, K, feat, reject, VK, W, api.rows, api.row0)
            same(C_dev, Cp, (what, f, "C")), same(VC_dev, VC, (what, f, "VC"))
            assert (VC[:, :3] > 0).any()
        else:
            assert not C_dev.any() and not VC_dev.any()
        same(blend, capi.history_blend_host(S, SPP, Cp), (what, f, "blend"))
        same(filtered, capi.history_denoise_host(S, feat, noise, W, api.rows, GROUPS, SPP, SPP, Cp, VC), (what, f, "pt_history_denoise"))
        K, VK, kept_cam = capi.history_capture_host(S, feat, SPP, Cp), capi.history_capture_variance_host(noise, GROUPS, SPP, SPP, Cp, VC), cam
        same(K_dev, K, (what, f, "K")), same(VK_dev, VK, (what, f, "VK"))
    assert (VK[:, :3] > 0).any() and not VK[:, 3].any()


@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
def test_renderer_sequence_equals_host_through_two_moves(orbit_paths, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    api = Default(scene, arith=arith)
    try:
        seen, made = sequence(api, orbit_paths, 3)
    finally:
        api.free()
    check_against_host(api, scene, seen, made, arith)


def test_a_tile_of_rows_10_to_40_through_a_context(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    api = Context(scene, 10, 31)
    try:
        seen, made = sequence(api, orbit_paths, 3)
        # the _device form names the filtered image inside the workspace
        dev = C.c_void_p()
        api.call("history_denoise_device", C.c_float(SPP), None, C.byref(dev))
        assert dev.value
    finally:
        api.free()
    check_against_host(api, scene, seen, made, "tile")


@pytest.mark.parametrize("w,rows", [(97, 61), (5, 3)])
def test_stage_equals_host(scene_dir, w, rows):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = w * rows
    groups, iters = 3, 4
    _, planes = denoise_ref.random_frame(w, rows, iters)
    noise = denoise_guided_ref.random_noise_planes(w, rows, groups, iters)
    S = noise[0, :, :3]
    cam, kept, feat, reject, _ = href.adversarial(w, rows, 7)
    rng = np.random.default_rng(n)
    vk = np.zeros((n, 4), f32)
    vk[:, :3] = rng.random((n, 3), dtype=f32) * f32(0.01)
    vk[rng.random(n) < 0.2] = 0
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(32, 24)))
    try:
        for name, opts in href.OPTION_SETS.items():
            Cp, VC = capi.stage_history_reproject_variance(cam.to_capi(), kept, feat, reject, vk, w, rows, 7, **opts)
            want_C, want_VC = capi.history_reproject_variance_host(cam.to_capi(), kept, feat, reject, vk, w, rows, 7, **opts)
            same(Cp, want_C, (w, rows, name, "C")), same(VC, want_VC, (w, rows, name, "VC"))
        Cp, VC = capi.history_reproject_variance_host(cam.to_capi(), kept, feat, reject, vk, w, rows, 7)
        for opts in (dict(), dict(keep_albedo=True), dict(levels=2, sigma_color=2.0)):
            same(capi.stage_history_denoise(S, planes, noise, w, rows, groups, iters, iters, Cp, VC, **opts),
                 capi.history_denoise_host(S, planes, noise, w, rows, groups, iters, iters, Cp, VC, **opts), (w, rows, opts))
        same(capi.stage_history_denoise(S, planes, noise, w, rows, groups, iters, iters),
             capi.denoise_guided_host(S, planes, noise, w, rows, groups, iters), (w, rows, "C absent: the guided filter"))
    finally:
        r.free()


def folded_view(r, first=1):
    for g in range(GROUPS):
        r.render(first + g, 1)
        r.noise_fold()
    r.render_features(1, 1)


def test_flags_0_is_the_old_call(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    planes, bytes_ = [], []
    for ex in (False, True):
        r = capi.Renderer(capi.Scene(orbit_paths[0], res=RES))
        try:
            folded_view(r)
            r.history_capture_ex(SPP, 0) if ex else r.history_capture(SPP)
            r.set_camera(capi.Scene(orbit_paths[1], res=RES).camera)
            folded_view(r, SPP + 1)
            r.history_reproject_ex(0) if ex else r.history_reproject()
            resolved = r.history_resolve(SPP)
            r.history_capture_ex(SPP, 0) if ex else r.history_capture(SPP)
            planes.append(r.readback_history() + (resolved,))
            bytes_.append(r.stats().device_bytes)
            vk, vc = r.readback_history_variance()
            assert not vk.any() and not vc.any()  # absent: zeros, and nothing allocated for them
            assert r.stats().device_bytes == bytes_[-1]
        finally:
            r.free()
    for a, b, name in zip(planes[0], planes[1], ("K", "C", "resolve")):
        same(b, a, name)
    assert bytes_[0] == bytes_[1]


def test_lifetimes_and_device_bytes(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = W * H
    r = capi.Renderer(capi.Scene(orbit_paths[0], res=RES))
    try:
        folded_view(r)
        r.history_capture(SPP)
        before = r.stats().device_bytes
        r.history_capture_ex(SPP)
        assert r.stats().device_bytes - before == 32 * n  # the first capture with variance, and only that
        r.history_reproject_ex()  # standing still
        r.history_capture_ex(SPP)
        r.history_reproject_ex()
        assert r.stats().device_bytes - before == 32 * n + 16  # (+ reject_geom: 7 geoms, an allocation holds at least 16 bytes)
        vk, vc = r.readback_history_variance()
        assert (vk[:, :3] > 0).any() and (vc[:, :3] > 0).any() and not vk[:, 3].any() and not vc[:, 3].any()
        assert not r.readback_history()[0][2, :, 3].any()  # K2.w stays +0
        for move in (lambda: r.clear(), lambda: r.set_camera(capi.Scene(orbit_paths[1], res=RES).camera),
                     lambda: r.set_camera(capi.Scene(orbit_paths[2], res=RES).camera, device_tables=True)):
            move()
            k, c = r.readback_history_variance()
            same(k, vk, "VK survives")
            assert not c.any()  # VC is absent, like C
            folded_view(r)
            r.history_reproject_ex()
            assert (r.readback_history_variance()[1][:, :3] > 0).any()
        after_moves = r.stats().device_bytes  # (the move with device tables allocated its own buffers)
        # a plain lookup leaves C without VC; a plain capture leaves K without variance
        r.history_reproject()
        assert not r.readback_history_variance()[1].any() and (r.readback_history()[1][:, 3] > 0).any()
        with pytest.raises(capi.PtError, match="pt_history_capture_ex: the current plane has no variance"):
            r.history_capture_ex(SPP)
        with pytest.raises(capi.PtError, match="pt_history_denoise: the current plane has no variance"):
            r.history_denoise(SPP)
        r.history_capture(SPP)
        assert not r.readback_history_variance()[0].any()
        with pytest.raises(capi.PtError, match="pt_history_reproject_ex: nothing has been captured with variance"):
            r.history_reproject_ex()
        r.history_reproject()
        r.clear()
        folded_view(r)
        r.history_capture_ex(SPP)
        r.history_reproject_ex()
        r.history_drop()
        k, c = r.readback_history_variance()
        assert not k.any() and not c.any()
        with pytest.raises(capi.PtError, match="pt_history_reproject_ex: nothing has been captured"):
            r.history_reproject_ex()
        assert r.stats().device_bytes == after_moves  # nothing freed, nothing more allocated
    finally:
        r.free()


def test_refusals_by_name_phrase_and_order(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    L = capi.lib()
    n = W * H
    buf = np.empty((n, 3), f32)
    p = capi._f(buf)

    def refused(rc, *phrases):
        assert rc != 0
        msg = L.pt_last_error().decode()
        for ph in phrases:
            assert ph in msg, (ph, msg)

    capi.pt_free()
    refused(L.pt_history_capture_ex(C.c_float(4.0), 2), "pt_history_capture_ex", "pt_init")
    refused(L.pt_history_reproject_ex(None, 2), "pt_history_reproject_ex", "pt_init")
    refused(L.pt_history_denoise(C.c_float(4.0), None, None), "pt_history_denoise", "pt_init")
    refused(L.pt_readback_history_variance(None, None), "pt_readback_history_variance", "pt_init")
    # the undefined flag bit comes before the ragged tile; the ragged tile before everything else
    r = capi.Renderer(scene, pixel_begin=10, pixel_count=W * 3)
    try:
        before = r.stats().device_bytes
        refused(L.pt_history_capture_ex(C.c_float(-1.0), 3), "pt_history_capture_ex", "flag")
        refused(L.pt_history_reproject_ex(None, 0x80000000), "pt_history_reproject_ex", "flag")
        refused(L.pt_history_capture_ex(C.c_float(-1.0), VAR), "pt_history_capture_ex", "whole contiguous image rows")
        refused(L.pt_history_reproject_ex(None, VAR), "pt_history_reproject_ex", "whole contiguous image rows")
        refused(L.pt_history_denoise(C.c_float(-1.0), None, None), "pt_history_denoise", "whole contiguous image rows")
        assert r.stats().device_bytes == before
    finally:
        r.free()
    r = capi.Renderer(scene)
    try:
        before = r.stats().device_bytes
        bad_dn = capi.PtDenoiseOptions(9, 0.0, 0.0, 0.0, 0)
        bad_hi = capi.PtHistoryOptions(-1.0, 0.0, 0.0, 0)
        # the old function's refusals in their order, under the new name
        refused(L.pt_history_capture_ex(C.c_float(-1.0), VAR), "pt_history_capture_ex", "no feature pass")
        refused(L.pt_history_reproject_ex(C.byref(bad_hi), VAR), "pt_history_reproject_ex", "nothing has been captured")
        refused(L.pt_history_denoise(C.c_float(-1.0), C.byref(bad_dn), None), "pt_history_denoise", "no feature pass")
        assert r.stats().device_bytes == before
        r.render_features(1, 1)
        before = r.stats().device_bytes
        refused(L.pt_history_capture_ex(C.c_float(-1.0), VAR), "pt_history_capture_ex", "samples")
        # then the variance's own: nothing folded, fewer than 2 groups, fold first, samples != T
        refused(L.pt_history_capture_ex(C.c_float(4.0), VAR), "pt_history_capture_ex", "nothing has been folded")
        refused(L.pt_history_denoise(C.c_float(-1.0), C.byref(bad_dn), None), "pt_history_denoise", "samples")
        refused(L.pt_history_denoise(C.c_float(4.0), C.byref(bad_dn), None), "pt_history_denoise", "levels")
        refused(L.pt_history_denoise(C.c_float(4.0), C.byref(capi.PtDenoiseOptions(0, float("nan"), 0.0, 0.0, 0)), None), "pt_history_denoise", "sigma")
        refused(L.pt_history_denoise(C.c_float(4.0), C.byref(capi.PtDenoiseOptions(0, 0.0, 0.0, 0.0, 2)), None), "pt_history_denoise", "keep_albedo")
        refused(L.pt_history_denoise(C.c_float(4.0), None, None), "pt_history_denoise", "nothing has been folded")
        assert r.stats().device_bytes == before
        r.render(1, 2)
        r.noise_fold()
        before = r.stats().device_bytes  # (the fold's planes)
        refused(L.pt_history_capture_ex(C.c_float(4.0), VAR), "pt_history_capture_ex", "1 group(s) folded")
        refused(L.pt_history_denoise(C.c_float(4.0), None, None), "pt_history_denoise", "1 group(s) folded")
        r.render(3, 1)
        r.noise_fold()
        r.render(4, 1)
        refused(L.pt_history_capture_ex(C.c_float(5.0), VAR), "pt_history_capture_ex", "fold first")
        refused(L.pt_history_denoise(C.c_float(5.0), None, None), "pt_history_denoise", "fold first")
        r.noise_fold()
        refused(L.pt_history_capture_ex(C.c_float(5.0), VAR), "pt_history_capture_ex", "samples 5", "4 iterations")
        refused(L.pt_history_denoise(C.c_float(5.0), None, None), "pt_history_denoise", "samples 5", "4 iterations")
        refused(L.pt_history_denoise(C.c_float(4.0), None, None), "pt_history_denoise", "null")
        assert r.stats().device_bytes == before  # nothing allocated by any of them
        r.history_capture(SPP)  # kept without variance
        refused(L.pt_history_reproject_ex(C.byref(bad_hi), VAR), "pt_history_reproject_ex", "cap")  # the options come first
        refused(L.pt_history_reproject_ex(None, VAR), "pt_history_reproject_ex", "nothing has been captured with variance")
        r.history_reproject()
        # C without VC: after the folds' conditions, before the null buffer
        refused(L.pt_history_capture_ex(C.c_float(5.0), VAR), "pt_history_capture_ex", "samples 5")
        refused(L.pt_history_capture_ex(C.c_float(4.0), VAR), "pt_history_capture_ex", "the current plane has no variance", "PT_HISTORY_VARIANCE")
        refused(L.pt_history_denoise(C.c_float(4.0), None, None), "pt_history_denoise", "the current plane has no variance")
        # flags == 0 through the _ex forms still refuses what the old calls refuse, and only that
        r.clear()
        refused(L.pt_history_reproject_ex(None, 0), "pt_history_reproject_ex", "no feature pass")
        r.render_features(1, 1)
        r.render(1, 1)
        assert L.pt_history_capture_ex(C.c_float(1.0), 0) == 0 and L.pt_history_reproject_ex(None, 0) == 0  # no fold asked for
        # the adaptive state
        r.clear()
        for g in range(2):
            r.render(g * SPP + 1, SPP)
            r.noise_fold()
        r.render_features(1, 1)
        r.adaptive_round(2 * SPP + 1, SPP, 0.25)
        refused(L.pt_history_capture_ex(C.c_float(-1.0), VAR), "pt_history_capture_ex", "adaptive state")
        refused(L.pt_history_reproject_ex(C.byref(bad_hi), VAR), "pt_history_reproject_ex", "adaptive state")
        refused(L.pt_history_denoise(C.c_float(-1.0), C.byref(bad_dn), p), "pt_history_denoise", "adaptive state")
    finally:
        r.free()


def test_the_orbit_of_the_simulation_on_the_device(orbit_paths):
    """The exact build reproduces the oracle's samples bit for bit, so the orbit of tests/test_history_variance_sim.py run on the
    renderer gives the simulation's figures; the 1024-spp frame at the last camera comes from the renderer too."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    api = Default(capi.Scene(orbit_paths[0], res=RES), arith="exact")
    try:
        seen, made = sequence(api, orbit_paths, href.FRAMES, device_tables_at=-1)
    finally:
        api.free()
    r = capi.Renderer(capi.Scene(orbit_paths[-1], res=RES), arith="exact")
    try:
        for g in range(GROUPS):
            r.render((href.FRAMES - 1) * SPP + g + 1, 1)
            r.noise_fold()
        r.render_features(1, 1)
        alone_img = r.denoise_guided()
        r.clear()
        r.render(href.TRUTH_FIRST, href.TRUTH_SPP)
        truth = r.readback().astype(np.float64) / href.TRUTH_SPP
    finally:
        r.free()
    _, _, blend, filtered, _, VK = made[-1]
    carried, both, alone = href.mse(blend, truth), href.mse(filtered, truth), href.mse(alone_img, truth)
    sum_var, sum_err2 = ref.calibration(VK, blend, truth)
    print(f"orbit on the device, last view: MSE blend {carried:.6g}, filtered blend {both:.6g}, guided filter alone {alone:.6g}; "
          f"sum of the carried variance {sum_var:.6g} against {sum_err2:.6g}")
    assert both < carried and both < alone
    assert abs(carried - href.SIM_CARRIED) < 1e-7 and abs(both - ref.SIM_FILTERED) < 1e-7 and abs(alone - ref.SIM_GUIDED_ALONE) < 1e-7
    assert abs(sum_var / ref.SIM_SUM_VAR - 1) < 1e-7 and abs(sum_err2 / ref.SIM_SUM_ERR2 - 1) < 1e-7
