"""The reprojected sample history on the device (pt_history_capture / _reproject / _resolve, csrc/pt_history.hip) against the library's
host functions (the same bodies, csrc/pt_history.h; pinned to the numpy restatement by tests/test_history_host.py), bit for bit.  The
host functions are always fed with the renderer's own readbacks — pinned to the oracle by other tests — so these tests isolate the
history."""
import numpy as np
import pytest

import camera_scenes
import history_ref as ref
from history_ref import bits, f32

pytestmark = pytest.mark.gpu
RES, SPP = ref.RES, ref.SPP
N = RES[0] * RES[1]


def same(got, want, what):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


@pytest.fixture(scope="module")
def orbit_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_history")
    return dict(cornell=ref.orbit_scene_paths(d, camera_scenes.cornell_text), random=ref.orbit_scene_paths(d, camera_scenes.random_text, frames=3))


@pytest.mark.parametrize("row0", ref.ROW0)
@pytest.mark.parametrize("w,rows", ref.SHAPES)
def test_stage_equals_host(scene_dir, w, rows, row0):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    cam, kept, feat, reject, _ = ref.adversarial(w, rows, row0)
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(32, 24)))
    try:
        for name, opts in ref.OPTION_SETS.items():
            got = capi.stage_history_reproject(cam.to_capi(), kept, feat, reject, w, rows, row0, **opts)
            same(got, capi.history_reproject_host(cam.to_capi(), kept, feat, reject, w, rows, row0, **opts), (w, rows, row0, name))
    finally:
        r.free()


def renderer_sequence(paths, views, **kw):
    """The renderer through `views` views (the command line's order, every view its own iterations): per view the renderer's readbacks
    (camera, S, feature planes) and what it made of them (current plane after the reprojection, resolved image, kept planes)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(paths[0], res=RES)
    r = capi.Renderer(scene, **kw)
    seen, made = [], []
    try:
        for f in range(views):
            cam = capi.Scene(paths[f], res=RES).camera
            if f > 0:
                r.set_camera(cam, device_tables=(f == 2))
            r.render_features(1, 1)
            if f > 0:
                r.history_reproject()
            r.render(f * SPP + 1, SPP)
            resolved = r.history_resolve(SPP)
            _, current = r.readback_history() if f > 0 else (None, np.zeros((N, 4), f32))
            seen.append((cam, r.readback(), r.readback_feature_planes()))
            r.history_capture(SPP)
            kept, _ = r.readback_history()
            made.append((current, resolved, kept))
    finally:
        r.free()
    return scene, seen, made


@pytest.mark.parametrize("scene_name", ["cornell", "random"])
@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
def test_renderer_sequence_equals_host_through_two_moves(orbit_paths, arith, scene_name):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene, seen, made = renderer_sequence(orbit_paths[scene_name], 3, arith=arith)
    reject = capi.reject_geoms(scene)
    kept = kept_cam = None
    for f, ((cam, S, feat), (current, resolved, kept_dev)) in enumerate(zip(seen, made)):
        C = None if kept is None else capi.history_reproject_host(kept_cam, kept, feat, reject, RES[0], RES[1])
        if C is not None:
            same(current, C, (arith, scene_name, f, "current plane"))
            assert (C[:, 3] > 0).sum() > N // 10
        same(resolved, capi.history_blend_host(S, SPP, C), (arith, scene_name, f, "resolve"))
        kept, kept_cam = capi.history_capture_host(S, feat, SPP, C), cam
        same(kept_dev, kept, (arith, scene_name, f, "kept planes"))
    assert (made[2][2][0, :, 3] == 3 * SPP).any()  # pixels carried through both moves


def test_kept_planes_survive_clear_and_both_moves_and_the_current_plane_does_not(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    paths = orbit_paths["cornell"]
    r = capi.Renderer(capi.Scene(paths[0], res=RES))
    try:
        r.render(1, SPP)
        r.render_features(1, 1)
        r.history_capture(SPP)
        r.history_reproject()  # standing still
        kept, current = r.readback_history()
        assert (current[:, 3] > 0).any() and (kept[0, :, 3] == SPP).all()
        for move in (lambda: r.clear(), lambda: r.set_camera(capi.Scene(paths[1], res=RES).camera),
                     lambda: r.set_camera(capi.Scene(paths[2], res=RES).camera, device_tables=True)):
            move()
            k, c = r.readback_history()
            same(k, kept, "kept planes")
            assert not c.any()
            same(r.history_resolve(SPP), np.zeros((N, 3), f32), "nothing rendered, C absent")
            r.render_features(1, 1)
            r.history_reproject()
            assert (r.readback_history()[1][:, 3] > 0).any()
        r.history_drop()
        k, c = r.readback_history()
        assert not k.any() and not c.any()
        with pytest.raises(capi.PtError, match="pt_history_reproject: nothing has been captured"):
            r.history_reproject()
    finally:
        r.free()


def test_device_bytes_grow_by_64_per_pixel_at_the_first_capture_only(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    paths = orbit_paths["cornell"]
    scene = capi.Scene(paths[0], res=RES)
    r = capi.Renderer(scene)
    try:
        r.render(1, SPP)
        r.render_features(1, 1)
        r.history_resolve(SPP)  # (the resolve's own buffer, pt_resolve's)
        before = r.stats().device_bytes
        r.history_capture(SPP)
        assert r.stats().device_bytes - before == 64 * N
        r.history_capture(SPP)
        r.clear()
        r.render(1, SPP)
        r.render_features(1, 1)
        r.history_capture(SPP)
        assert r.stats().device_bytes - before == 64 * N
        r.history_reproject()  # the first reprojection adds reject_geom, one byte per geom (an allocation holds at least 16)
        assert r.stats().device_bytes - before == 64 * N + max(len(scene.geoms()), 16)
        r.history_reproject()
        r.history_drop()
        assert r.stats().device_bytes - before == 64 * N + max(len(scene.geoms()), 16)
    finally:
        r.free()
    r = capi.Renderer(scene)
    try:
        r.render(1, SPP)
        first = r.stats().device_bytes
        r.render_features(1, 1)
        after_features = r.stats().device_bytes
        r.clear()
        r.set_camera(capi.Scene(paths[1], res=RES).camera)
        r.render(1, SPP)
        r.render_features(1, 1)
        assert r.stats().device_bytes == after_features and after_features - first == 48 * N
    finally:
        r.free()


def test_refusals_by_name_phrase_and_order(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    import ctypes as C
    paths = orbit_paths["cornell"]
    scene = capi.Scene(paths[0], res=RES)
    L = capi.lib()
    out = np.empty((N, 3), f32)

    def refused(rc, *phrases):
        assert rc != 0
        msg = L.pt_last_error().decode()
        for p in phrases:
            assert p in msg, (p, msg)

    capi.pt_free()
    # no renderer
    refused(L.pt_history_capture(C.c_float(4.0)), "pt_history_capture", "pt_init")
    refused(L.pt_history_reproject(None), "pt_history_reproject", "pt_init")
    refused(L.pt_history_resolve(C.c_float(4.0), capi._f(out)), "pt_history_resolve", "pt_init")
    refused(L.pt_readback_history(None, None), "pt_readback_history", "pt_init")
    refused(L.pt_history_drop(), "pt_history_drop", "pt_init")
    # a ragged tile comes before everything else an argument could break
    r = capi.Renderer(scene, pixel_begin=10, pixel_count=RES[0] * 3)
    try:
        before = r.stats().device_bytes
        refused(L.pt_history_capture(C.c_float(-1.0)), "pt_history_capture", "whole contiguous image rows")
        refused(L.pt_history_reproject(None), "pt_history_reproject", "whole contiguous image rows")
        refused(L.pt_history_resolve(C.c_float(-1.0), None), "pt_history_resolve", "whole contiguous image rows")
        assert r.stats().device_bytes == before
    finally:
        r.free()
    r = capi.Renderer(scene)
    try:
        before = r.stats().device_bytes
        # capture: features, then samples
        refused(L.pt_history_capture(C.c_float(-1.0)), "pt_history_capture", "no feature pass")
        refused(L.pt_history_reproject(None), "pt_history_reproject", "nothing has been captured")
        assert r.stats().device_bytes == before
        r.render(1, SPP)
        r.render_features(1, 1)
        before = r.stats().device_bytes
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused(L.pt_history_capture(C.c_float(bad)), "pt_history_capture", "samples")
        # resolve: samples, then the null pointer
        refused(L.pt_history_resolve(C.c_float(0.0), None), "pt_history_resolve", "samples")
        refused(L.pt_history_resolve(C.c_float(4.0), None), "pt_history_resolve", "null")
        assert r.stats().device_bytes == before  # nothing allocated by any of them
        r.history_capture(SPP)
        # reproject: captured, then the feature pass since the last clear or move, then the options
        r.clear()
        bad_opt = capi.PtHistoryOptions(-1.0, 0.0, 0.0, 0)
        refused(L.pt_history_reproject(C.byref(bad_opt)), "pt_history_reproject", "no feature pass")
        refused(L.pt_history_capture(C.c_float(4.0)), "pt_history_capture", "no feature pass")
        r.render_features(1, 1)
        refused(L.pt_history_reproject(C.byref(bad_opt)), "pt_history_reproject", "cap")
        for opt in (capi.PtHistoryOptions(float("nan"), 0, 0, 0), capi.PtHistoryOptions(0, float("inf"), 0, 0), capi.PtHistoryOptions(0, 0, float("nan"), 0),
                    capi.PtHistoryOptions(0, 0, 0, 2)):
            refused(L.pt_history_reproject(C.byref(opt)), "pt_history_reproject")
        r.set_camera(capi.Scene(paths[1], res=RES).camera)
        refused(L.pt_history_reproject(None), "pt_history_reproject", "no feature pass")
        # the adaptive state: the message names pt_resolve and pt_clear
        r.clear()
        for g in range(2):
            r.render(g * SPP + 1, SPP)
            r.noise_fold()
        r.render_features(1, 1)
        r.adaptive_round(2 * SPP + 1, SPP, 0.25)
        refused(L.pt_history_capture(C.c_float(-1.0)), "pt_history_capture", "adaptive state", "pt_resolve", "pt_clear")
        refused(L.pt_history_reproject(C.byref(bad_opt)), "pt_history_reproject", "adaptive state", "pt_resolve", "pt_clear")
        refused(L.pt_history_resolve(C.c_float(-1.0), None), "pt_history_resolve", "adaptive state", "pt_resolve", "pt_clear")
    finally:
        r.free()


def test_the_orbit_of_the_simulation_on_the_device(orbit_paths):
    """The exact build reproduces the oracle's samples bit for bit, so the orbit of tests/test_history_sim.py run on the renderer gives
    the simulation's figures; the 1024-spp frame and the 32 uniform spp at the last camera come from the renderer too."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    paths = orbit_paths["cornell"]
    _, seen, made = renderer_sequence(paths, ref.FRAMES, arith="exact")
    r = capi.Renderer(capi.Scene(paths[-1], res=RES), arith="exact")
    try:
        r.render(1, ref.UNIFORM_SPP)
        uniform = r.readback().astype(np.float64) / ref.UNIFORM_SPP
        r.clear()
        r.render(ref.TRUTH_FIRST, ref.TRUTH_SPP)
        truth = r.readback().astype(np.float64) / ref.TRUTH_SPP
    finally:
        r.free()
    raw = ref.mse(seen[-1][1].astype(np.float64) / SPP, truth)
    carried = ref.mse(made[-1][1], truth)
    print(f"orbit on the device, last view: MSE raw {raw:.6g}, {ref.UNIFORM_SPP} uniform spp {ref.mse(uniform, truth):.6g}, reprojected {carried:.6g} ({carried / raw:.4f} of raw)")
    assert carried < 0.5 * raw
    assert abs(raw - ref.SIM_RAW) < 1e-7 and abs(ref.mse(uniform, truth) - ref.SIM_UNIFORM) < 1e-7 and abs(carried - ref.SIM_CARRIED) < 1e-7
