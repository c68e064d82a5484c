"""Moments with the history on the device (pt_history_capture_ex / _reproject_ex with PT_HISTORY_MOMENTS, pt_history_denoise_ex;
csrc/pt_history.hip, csrc/pt_denoise.hip with k_denoise_var_spatial) against the library's host functions (the same bodies; pinned to
the numpy restatement by tests/test_history_moments_host.py), bit for bit.  The host functions are always fed with the renderer's own
readbacks, so these tests isolate the new code."""
import ctypes as C

import numpy as np
import pytest

import camera_scenes
import denoise_ref
import history_ref as href
import history_moments_ref as ref
from history_ref import bits, f32

pytestmark = pytest.mark.gpu
RES = href.RES
W, H = RES
VAR, MOM = 1, 2  # PT_HISTORY_VARIANCE, PT_HISTORY_MOMENTS
SPP = 1

# the window (7 x 7) is larger than the frame; the wave and block edges of a 64 x 4 tile; more than one block each way with row0 > 0
STAGE_SHAPES = [(1, 1, 0), (2, 2, 0), (5, 3, 0), (63, 5, 0), (64, 4, 0), (65, 9, 0), (97, 61, 7)]


def same(got, want, what):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


@pytest.fixture(scope="module")
def orbit_paths(tmp_path_factory):
    return href.orbit_scene_paths(tmp_path_factory.mktemp("gpu_history_moments"), camera_scenes.cornell_text)


def kept_moments(n, seed):
    rng = np.random.default_rng(seed)
    vk = np.zeros((n, 4), f32)
    vk[:, :3] = rng.random((n, 3), dtype=f32) * f32(0.01)
    vk[:, 3] = rng.choice(np.array([1.0, 0.5, 0.25, 0.125], f32), n)
    vk[rng.random(n) < 0.2] = 0
    return vk


@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
def test_stage_equals_host(scene_dir, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(32, 24)), arith=arith)
    try:
        for w, rows, row0 in STAGE_SHAPES:
            n = w * rows
            cam, kept, feat, reject, _ = href.adversarial(w, rows, row0)
            vk = kept_moments(n, n)
            for name, opts in href.OPTION_SETS.items():
                Cp, VC = capi.stage_history_reproject_moments(cam.to_capi(), kept, feat, reject, vk, w, rows, row0, **opts)
                want_C, want_VC = capi.history_reproject_moments_host(cam.to_capi(), kept, feat, reject, vk, w, rows, row0, **opts)
                same(Cp, want_C, (w, rows, name, "C")), same(VC, want_VC, (w, rows, name, "VC"))
            if n > 1000:
                assert (want_VC[:, 3] > 0).any()
            S, planes = denoise_ref.random_frame(w, rows, SPP)
            for pattern in ref.MARK_PATTERNS:
                Cp, VC, marked = ref.current_planes(w, rows, pattern)
                for opts in (dict(levels=2), dict(levels=1, keep_albedo=True, sigma_normal=-1.0)):
                    st = {}
                    want = capi.history_denoise_moments_host(S, planes, w, rows, SPP, Cp, VC, stats=st, **opts)
                    assert np.array_equal(st["mark"], marked)
                    same(capi.stage_history_denoise_moments(S, planes, w, rows, SPP, Cp, VC, **opts), want, (w, rows, pattern, opts))
            same(capi.stage_history_denoise_moments(S, planes, w, rows, SPP), capi.history_denoise_moments_host(S, planes, w, rows, SPP),
                 (w, rows, "C absent: every pixel marked, default options"))
    finally:
        r.free()


def history_readbacks(r):
    K, Cp = r.readback_history()
    VK, VC = r.readback_history_variance()
    return K, Cp, VK, VC


def sequence(capi, r, paths, views):
    """The command line's --denoise-history --history-moments order through `views` views at 1 spp: per view what the renderer read
    back (camera, S, features) and what it made of them (C, VC, blend, filtered blend, K, VK)."""
    n = W * H
    seen, made = [], []
    for f in range(views):
        cam = capi.Scene(paths[f], res=RES).camera
        if f > 0:
            r.set_camera(cam)
        r.render(f * SPP + 1, SPP)
        r.render_features(1, 1)
        if f > 0:
            r.history_reproject_ex(MOM)
        blend = r.history_resolve(SPP)
        filtered = r.history_denoise_ex(SPP)
        if f > 0:
            _, Cp, _, VC = history_readbacks(r)
        else:  # nothing captured yet: pt_readback_history refuses, the other readback gives zeros
            Cp, VC = np.zeros((n, 4), f32), r.readback_history_variance()[1]
        seen.append((cam, r.readback(), r.readback_feature_planes()))
        r.history_capture_ex(SPP, MOM)
        K, _, VK, _ = history_readbacks(r)
        made.append((Cp, VC, blend, filtered, K, VK))
    return seen, made


def check_against_host(capi, scene, seen, made):
    reject = capi.reject_geoms(scene)
    K = VK = kept_cam = None
    for f, ((cam, S, feat), (C_dev, VC_dev, blend, filtered, K_dev, VK_dev)) in enumerate(zip(seen, made)):
        Cp = VC = None
        if K is not None:
            Cp, VC = capi.history_reproject_moments_host(kept_cam, K, feat, reject, VK, W, H)
            same(C_dev, Cp, (f, "C")), same(VC_dev, VC, (f, "VC"))
            assert (VC[:, 3] > 0).any()
        else:
            assert not C_dev.any() and not VC_dev.any()
        same(blend, capi.history_blend_host(S, SPP, Cp), (f, "blend"))
        same(filtered, capi.history_denoise_moments_host(S, feat, W, H, SPP, Cp, VC), (f, "pt_history_denoise_ex"))
        K, VK, kept_cam = capi.history_capture_host(S, feat, SPP, Cp), capi.history_capture_moments_host(S, SPP, Cp, VC), cam
        same(K_dev, K, (f, "K")), same(VK_dev, VK, (f, "VK"))
    assert (VK[:, 3] < 1).any() and (VK[:, 3] > 0).all()


def test_renderer_sequence_equals_host(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    r = capi.Renderer(scene, arith="exact")
    try:
        seen, made = sequence(capi, r, orbit_paths, 3)
    finally:
        r.free()
    check_against_host(capi, scene, seen, made)


def test_the_orbit_of_the_simulation_on_the_device(orbit_paths):
    """The exact build reproduces the oracle's samples bit for bit, so the orbit of tests/test_history_moments_sim.py run on the
    renderer gives the simulation's figures; the 1024-spp frame at the last camera comes from the renderer too."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(orbit_paths[0], res=RES), arith="exact")
    try:
        seen, made = sequence(capi, r, orbit_paths, href.FRAMES)
    finally:
        r.free()
    r = capi.Renderer(capi.Scene(orbit_paths[-1], res=RES), arith="exact")
    try:
        r.render(href.FRAMES, 1)
        r.render_features(1, 1)
        alone_img = r.denoise(1)
        r.clear()
        r.render(href.TRUTH_FIRST, href.TRUTH_SPP)
        truth = r.readback().astype(np.float64) / href.TRUTH_SPP
    finally:
        r.free()
    (_, S, feat), (Cp, VC, blend, filtered, _, _) = seen[-1], made[-1]
    st = {}
    capi.history_denoise_moments_host(S, feat, W, H, SPP, Cp, VC, stats=st)
    without = href.mse(ref.denoise_moments(S, feat, W, H, SPP, Cp, VC, spatial=False), truth)
    hit = np.asarray(feat, f32).reshape(3, -1, 4)[1, :, 3] > 0
    carried, both, alone = href.mse(blend, truth), href.mse(filtered, truth), href.mse(alone_img, truth)
    share, err_share = ref.marked_share(st["mark"], hit, blend, truth)
    print(f"orbit at 1 spp on the device, last view: MSE blend {carried:.9g}, filtered blend {both:.9g}, pt_denoise alone {alone:.9g}, without the "
          f"spatial estimate {without:.9g}; marked hit pixels {share:.9g} with {err_share:.9g} of the squared error")
    assert both < carried and both < alone and both < without
    for got, pinned in ((carried, ref.SIM_BLEND), (both, ref.SIM_FILTERED), (alone, ref.SIM_PLAIN_ALONE), (without, ref.SIM_NO_SPATIAL),
                        (share, ref.SIM_MARKED_SHARE), (err_share, ref.SIM_MARKED_ERR_SHARE)):
        assert abs(got / pinned - 1) < 1e-6, (got, pinned)


def one_view(r, first=1):
    r.render(first, 1)
    r.render_features(1, 1)


def test_device_bytes_and_kinds_do_not_mix(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = W * H
    # a renderer using only the old calls: the same bytes with and without the moments kind in the library — the plain and the variance
    # calls allocate what they allocated (tests/test_gpu_history_variance.py pins 64 and 32 bytes per pixel)
    r = capi.Renderer(capi.Scene(orbit_paths[0], res=RES))
    try:
        one_view(r)
        before = r.stats().device_bytes
        r.history_capture(SPP)
        assert r.stats().device_bytes - before == 64 * n
        r.history_capture_ex(SPP, MOM)
        assert r.stats().device_bytes - before == 64 * n + 32 * n  # the first capture with moments, and only that
        vk, vc = r.readback_history_variance()
        x = (r.readback() / f32(SPP)).astype(f32)
        same(vk[:, :3], x * x, "VK of one view")
        assert (vk[:, 3] == 1).all() and not vc.any()
        r.history_reproject_ex(MOM)  # standing still
        r.history_capture_ex(SPP, MOM)
        r.history_reproject_ex(MOM)
        assert r.stats().device_bytes - before == 96 * n + 16  # (+ reject_geom: 7 geoms, an allocation holds at least 16 bytes)
        first = r.stats().device_bytes
        r.history_denoise_ex(SPP)
        workspace = r.stats().device_bytes - first
        r.history_denoise_ex(SPP)
        assert r.stats().device_bytes - first == workspace  # the shared 80 bytes per pixel, once
        # the variance kind reuses the buffer; the kinds do not mix across lookup and capture
        with pytest.raises(capi.PtError, match="pt_history_reproject_ex: nothing has been captured with variance"):
            r.history_reproject_ex(VAR)
        for g in range(2):
            r.render(2 + g, 1)
            r.noise_fold()
        folded = r.stats().device_bytes  # (the fold's planes)
        r.render_features(1, 1)
        r.history_reproject_ex(MOM)
        with pytest.raises(capi.PtError, match="pt_history_capture_ex: the current plane has no variance"):
            r.history_capture_ex(3, VAR)
        with pytest.raises(capi.PtError, match="pt_history_denoise: the current plane has no variance"):
            r.history_denoise(3)
        r.history_reproject()
        with pytest.raises(capi.PtError, match="pt_history_capture_ex: the current plane has no moments"):
            r.history_capture_ex(3, MOM)
        with pytest.raises(capi.PtError, match="pt_history_denoise_ex: the current plane has no moments"):
            r.history_denoise_ex(3)
        r.clear()
        for g in range(2):
            r.render(1 + g, 1)
            r.noise_fold()
        r.render_features(1, 1)
        r.history_capture_ex(2, VAR)  # C absent: any kind may follow
        with pytest.raises(capi.PtError, match="pt_history_reproject_ex: nothing has been captured with moments"):
            r.history_reproject_ex(MOM)
        r.history_reproject_ex(VAR)
        with pytest.raises(capi.PtError, match="pt_history_capture_ex: the current plane has no moments"):
            r.history_capture_ex(2, MOM)
        with pytest.raises(capi.PtError, match="pt_history_denoise_ex: the current plane has no moments"):
            r.history_denoise_ex(2)
        r.history_denoise(2)
        assert r.stats().device_bytes == folded  # nothing more allocated by any of it: one buffer serves both kinds
        # flags == 0 of the _ex filter is pt_history_denoise, bit for bit
        same(r.history_denoise_ex(2, 0), r.history_denoise(2), "flags == 0")
    finally:
        r.free()


def test_refusals_by_name_phrase_and_order(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    L = capi.lib()
    buf = np.empty((W * H, 3), f32)
    p = capi._f(buf)

    def refused(rc, *phrases):
        assert rc != 0
        msg = L.pt_last_error().decode()
        for ph in phrases:
            assert ph in msg, (ph, msg)

    who = "pt_history_denoise_ex"
    capi.pt_free()
    refused(L.pt_history_denoise_ex(C.c_float(1.0), None, 4, None), who, "pt_init")
    # the flag word comes before the ragged tile; the ragged tile before everything else
    r = capi.Renderer(scene, pixel_begin=10, pixel_count=W * 3)
    try:
        before = r.stats().device_bytes
        refused(L.pt_history_capture_ex(C.c_float(-1.0), VAR | MOM), "pt_history_capture_ex", "flag", "exclude each other")
        refused(L.pt_history_reproject_ex(None, VAR | MOM), "pt_history_reproject_ex", "flag", "exclude each other")
        refused(L.pt_history_capture_ex(C.c_float(-1.0), 4), "pt_history_capture_ex", "undefined flag")
        refused(L.pt_history_denoise_ex(C.c_float(-1.0), None, VAR, None), who, "undefined flag")
        refused(L.pt_history_denoise_ex(C.c_float(-1.0), None, VAR | MOM, None), who, "undefined flag")
        refused(L.pt_history_denoise_ex(C.c_float(-1.0), None, 0x80000000, None), who, "undefined flag")
        refused(L.pt_history_capture_ex(C.c_float(-1.0), MOM), "pt_history_capture_ex", "whole contiguous image rows")
        refused(L.pt_history_reproject_ex(None, MOM), "pt_history_reproject_ex", "whole contiguous image rows")
        refused(L.pt_history_denoise_ex(C.c_float(-1.0), None, MOM, None), who, "whole contiguous image rows")
        refused(L.pt_history_denoise_ex(C.c_float(-1.0), None, 0, None), who, "whole contiguous image rows")
        assert r.stats().device_bytes == before
    finally:
        r.free()
    r = capi.Renderer(scene)
    try:
        before = r.stats().device_bytes
        bad_dn = capi.PtDenoiseOptions(9, 0.0, 0.0, 0.0, 0)
        bad_hi = capi.PtHistoryOptions(-1.0, 0.0, 0.0, 0)
        refused(L.pt_history_capture_ex(C.c_float(-1.0), MOM), "pt_history_capture_ex", "no feature pass")
        refused(L.pt_history_reproject_ex(C.byref(bad_hi), MOM), "pt_history_reproject_ex", "nothing has been captured")
        refused(L.pt_history_denoise_ex(C.c_float(-1.0), C.byref(bad_dn), MOM, None), who, "no feature pass")
        refused(L.pt_history_denoise_ex(C.c_float(-1.0), C.byref(bad_dn), 0, None), who, "no feature pass")  # pt_history_denoise's, under the new name
        assert r.stats().device_bytes == before
        r.render(1, 1)
        r.render_features(1, 1)
        before = r.stats().device_bytes
        refused(L.pt_history_capture_ex(C.c_float(-1.0), MOM), "pt_history_capture_ex", "samples")
        refused(L.pt_history_denoise_ex(C.c_float(-1.0), C.byref(bad_dn), MOM, None), who, "samples")
        refused(L.pt_history_denoise_ex(C.c_float(1.0), C.byref(bad_dn), MOM, None), who, "levels")
        refused(L.pt_history_denoise_ex(C.c_float(1.0), C.byref(capi.PtDenoiseOptions(0, float("nan"), 0.0, 0.0, 0)), MOM, None), who, "sigma")
        refused(L.pt_history_denoise_ex(C.c_float(1.0), C.byref(capi.PtDenoiseOptions(0, 0.0, 0.0, 0.0, 2)), MOM, None), who, "keep_albedo")
        refused(L.pt_history_denoise_ex(C.c_float(1.0), None, MOM, None), who, "null")  # no fold condition stands before it
        refused(L.pt_history_denoise_ex(C.c_float(1.0), None, 0, None), who, "nothing has been folded")
        assert r.stats().device_bytes == before  # nothing allocated by any of them
        r.history_capture(SPP)  # kept without moments
        refused(L.pt_history_reproject_ex(C.byref(bad_hi), MOM), "pt_history_reproject_ex", "cap")  # the options come first
        refused(L.pt_history_reproject_ex(None, MOM), "pt_history_reproject_ex", "nothing has been captured with moments")
        r.history_reproject()
        # C of another kind: after samples and the options, before the null buffer
        refused(L.pt_history_capture_ex(C.c_float(-1.0), MOM), "pt_history_capture_ex", "samples")
        refused(L.pt_history_capture_ex(C.c_float(1.0), MOM), "pt_history_capture_ex", "the current plane has no moments", "PT_HISTORY_MOMENTS")
        refused(L.pt_history_denoise_ex(C.c_float(1.0), C.byref(bad_dn), MOM, None), who, "levels")
        refused(L.pt_history_denoise_ex(C.c_float(1.0), None, MOM, None), who, "the current plane has no moments")
        # the adaptive state
        r.clear()
        for g in range(2):
            r.render(g * 4 + 1, 4)
            r.noise_fold()
        r.render_features(1, 1)
        r.adaptive_round(9, 4, 0.25)
        refused(L.pt_history_capture_ex(C.c_float(-1.0), MOM), "pt_history_capture_ex", "adaptive state")
        refused(L.pt_history_reproject_ex(C.byref(bad_hi), MOM), "pt_history_reproject_ex", "adaptive state")
        refused(L.pt_history_denoise_ex(C.c_float(-1.0), C.byref(bad_dn), MOM, p), who, "adaptive state")
    finally:
        r.free()
