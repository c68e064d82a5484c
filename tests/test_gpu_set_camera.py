"""Moving the camera of a live renderer (pt_set_camera): after the move the renderer gives what a renderer freshly created at that
camera gives, bit for bit — image, feature planes, noise planes, adaptive rounds, filtered image, convergence curve — with the
tables, the grid, the worker and the batch buffers of the previous view gone.  The cameras are written into scene files so that the
library's loader and the oracle's apply the same fix-up."""
import ctypes as C

import numpy as np
import pytest

from camera_scenes import cornell_text, random_text, scene_path, stress_text

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def render_two_calls(r):
    r.render(1, 3)
    r.render(4, 5)
    return r.readback()


def fresh(path, features=False, **kw):
    """(image after iterations 1 .. 8 in two calls, stats[, feature planes]) of a renderer created for the scene file."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(path), **kw)
    try:
        img = render_two_calls(r)
        feat = None
        if features:
            r.render_features(1, 8)
            feat = r.readback_features()
        return img, r.stats(), feat
    finally:
        r.free()


# ---- cornell, every arithmetic mode, against a fresh renderer and the oracle ----------------------------------------------------
@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
def test_cornell_moved_equals_fresh_and_oracle(tmp_path, oracle, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    paths = {n: scene_path(tmp_path, cornell_text, n) for n in "ABE"}
    want = {n: fresh(paths[n], arith=arith)[0] for n in "ABE"}
    assert not np.array_equal(bits(want["A"]), bits(want["B"])) and not np.array_equal(bits(want["A"]), bits(want["E"]))
    r = capi.Renderer(capi.Scene(paths["A"]), arith=arith)
    try:
        assert np.array_equal(bits(render_two_calls(r)), bits(want["A"]))
        for n in "BEA":
            r.set_camera(capi.Scene(paths[n]).camera)
            got = render_two_calls(r)
            bad = np.flatnonzero((bits(got) != bits(want[n])).any(axis=1))
            assert bad.size == 0, (arith, n, bad.size, bad[:4], got[bad[:2]], want[n][bad[:2]])
            assert r.stats().samples == 96 * 54 * 8
            if arith == "exact":
                oracle.set_math_mode(oracle.PORTABLE)
                oracle.load_scene(paths[n])
                ref = oracle.render(1, 8, depth=8, variant=oracle.RETIRE, nthreads=16)
                assert np.array_equal(bits(got), bits(ref)), n
        assert r.setup_times().set_camera_calls == 3
    finally:
        r.free()


# ---- a scene with tightened leaves and, forced, a grid: tables, grid and statistics follow the camera ------------------------------
def grid_bytes(r, arith):
    """Device bytes of the grid the renderer walks: the cell table with its guard cells in front and behind, the 32-byte records, and
    in the fast build their centre / half extent copies; every allocation at least 16 bytes."""
    if not r.stats().grid_cells:
        return 0
    info, _ = r.grid_info()
    guard = info.res[0] * info.res[1] + info.res[0] + 2
    records = max(32 * info.num_records, 16)
    return 4 * (info.num_cells + 1 + 2 * guard) + records * (2 if arith == "fast" else 1)



@pytest.mark.parametrize("arith", ["exact", "fast"])
@pytest.mark.parametrize("flags", [0, 256])
def test_random_scene_tables_follow_the_camera(tmp_path, flags, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    order = "BCDEA"
    paths = {n: scene_path(tmp_path, random_text, n) for n in "ABCDE"}
    want = {n: fresh(paths[n], features=True, debug_flags=flags, arith=arith) for n in "ABCDE"}
    assert [want[n][1].tight_leaves for n in "ABCDE"] == [22, 21, 0, 0, 23]
    r = capi.Renderer(capi.Scene(paths["A"]), debug_flags=flags, arith=arith)
    try:
        render_two_calls(r)
        r.render_features(1, 8)
        base_bytes = r.stats().device_bytes - grid_bytes(r, arith)
        assert base_bytes + grid_bytes(r, arith) == want["A"][1].device_bytes
        for n in order:
            r.set_camera(capi.Scene(paths[n]).camera)
            img, st_fresh, feat = want[n]
            got = render_two_calls(r)
            assert np.array_equal(bits(got), bits(img)), (flags, arith, n)
            r.render_features(1, 8)
            got_feat = r.readback_features()
            for k in feat:
                assert np.array_equal(bits(got_feat[k]), bits(feat[k])), (flags, arith, n, k)
            st = r.stats()
            assert st.tight_leaves == st_fresh.tight_leaves, n
            # init's 4 x 4 x 4 cells also at C, where a fresh renderer's cost model says 3 x 3 x 3; none at D; back again after it
            assert st.grid_cells == (0 if not flags or n == "D" else 64), (flags, n)
            assert st_fresh.grid_cells == (0 if not flags or n == "D" else 27 if n == "C" else 64), (flags, n)
            # device memory moves by the size of the grid's tables and by nothing else
            assert st.device_bytes - grid_bytes(r, arith) == base_bytes, (flags, n)
            if n != "C":
                assert st.device_bytes == st_fresh.device_bytes, (flags, n)
    finally:
        r.free()


def test_stress_scene_keeps_the_structure_of_init(tmp_path):
    """Automatic choice: whatever the probe chose at init is walked after the move, at init's resolution (the cost model's
    candidate has 11 x 11 x 11 cells); the image is the fresh renderer's whatever that one chose."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    paths = {n: scene_path(tmp_path, stress_text, n) for n in "AB"}
    want, st_fresh, _ = fresh(paths["B"])
    assert st_fresh.tight_leaves == 62
    r = capi.Renderer(capi.Scene(paths["A"]))
    try:
        before = r.stats()
        assert before.tight_leaves == 149
        render_two_calls(r)
        r.set_camera(capi.Scene(paths["B"]).camera)
        after = r.stats()
        assert after.grid_cells == before.grid_cells and after.tight_leaves == 62
        assert np.array_equal(bits(render_two_calls(r)), bits(want))
        t = r.setup_times()
        assert t.set_camera_calls == 1 and t.set_camera_ms > 0 and t.tables_ms > 0 and t.probe_ms > 0
    finally:
        r.free()


# ---- state: everything accumulated is forgotten, and an existing worker follows the camera ---------------------------------------
THRESHOLD, FRACTION = 0.02, 0.25


def adaptive_sequence(r):
    """render, features, two folds, two threshold rounds (so that a worker exists), then what can be read."""
    out = {}
    r.render(1, 4)
    r.render_features(1, 4)
    r.noise_fold()
    r.render(5, 4)
    r.noise_fold()
    out["rounds"] = [r.adaptive_round_threshold(9, 4, THRESHOLD, FRACTION), r.adaptive_round_threshold(13, 4, THRESHOLD, FRACTION)]
    out["image"] = r.readback()
    noise = r.readback_noise()
    for k in noise:
        out["noise_" + k] = noise[k]
    out["counts"] = r.readback_adaptive()
    out["noise"] = r.noise()
    out["filtered"] = r.denoise_adaptive()
    return out


def same(a, b):
    if isinstance(a, np.ndarray):
        return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    return a == b


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_state_is_forgotten_and_the_worker_follows(tmp_path, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    paths = {n: scene_path(tmp_path, cornell_text, n) for n in "AB"}
    control = capi.Renderer(capi.Scene(paths["B"]), arith=arith)
    try:
        want = adaptive_sequence(control)
    finally:
        control.free()
    assert all(0 < m <= above for above, m in want["rounds"])  # the rounds rendered something: the worker ran
    r = capi.Renderer(capi.Scene(paths["A"]), arith=arith)
    try:
        at_a = adaptive_sequence(r)
        assert not same(at_a["image"], want["image"])
        r.set_camera(capi.Scene(paths["B"]).camera)
        assert not r.readback().any()
        assert r.stats().samples == 0
        assert r.noise() == dict(sse=-1.0, groups=0, iterations=0)
        assert not r.readback_adaptive().any()  # the uniform state, nothing folded
        feat = r.readback_features()
        assert all(not feat[k].any() for k in feat)
        got = adaptive_sequence(r)
        for k in want:
            assert same(got[k], want[k]), (arith, k)
    finally:
        r.free()


def test_convergence_is_rearmed(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    paths = {n: scene_path(tmp_path, cornell_text, n) for n in "AB"}
    control = capi.Renderer(capi.Scene(paths["B"]), convergence=2)
    try:
        control.render(1, 6)
        want = control.convergence(1, 6)
    finally:
        control.free()
    assert (want[:2] == -1).all() and (want[2:] >= 0).all()
    r = capi.Renderer(capi.Scene(paths["A"]), convergence=2)
    try:
        r.render(1, 6)
        assert (r.convergence(1, 6)[2:] >= 0).all()
        r.set_camera(capi.Scene(paths["B"]).camera)
        assert (r.convergence(1, 6) == -1).all() and r.iterations_to_clean(0.0) == -1  # the curve is forgotten
        r.render(1, 6)                                                                  # and the frame is captured again, at B
        assert np.array_equal(r.convergence(1, 6).view(np.uint64), want.view(np.uint64))
    finally:
        r.free()


# ---- refusals: by phrase, in order, with nothing changed ------------------------------------------------------------------------
def test_refusals(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(scene_path(tmp_path, cornell_text, "A"))
    moved = capi.Scene(scene_path(tmp_path, cornell_text, "B")).camera
    capi.pt_free()
    for cam in (None, C.byref(moved)):  # no renderer comes before a null camera
        assert capi.lib().pt_set_camera(cam) != 0
        assert b"pt_set_camera: pt_init has not been called" in capi.lib().pt_last_error()
    assert capi.lib().pt_get_setup_times(C.byref(capi.PtSetupTimes())) != 0
    r = capi.Renderer(scene)
    try:
        want = render_two_calls(r)
        bytes_before = r.stats().device_bytes

        def copy_of(cam):
            out = capi.PtCamera()
            C.memmove(C.byref(out), C.byref(cam), C.sizeof(out))
            return out

        assert capi.lib().pt_set_camera(None) != 0
        assert b"pt_set_camera: null camera" in capi.lib().pt_last_error()
        bad = copy_of(moved)
        bad.resolution[0] = 97
        bad.position[1] = float("nan")  # the resolution is looked at before the components
        with pytest.raises(capi.PtError, match=r"pt_set_camera: resolution 97x54 differs from the renderer's 96x54.*pt_init"):
            r.set_camera(bad)
        for field, n in (("position", 3), ("view", 3), ("up", 3), ("right", 3), ("fov", 2), ("pixelLength", 2)):
            for i, value in zip(range(n), (float("nan"), float("inf"), -float("inf"))):
                bad = copy_of(moved)
                getattr(bad, field)[i] = value
                with pytest.raises(capi.PtError, match=rf"pt_set_camera: camera {field}\[{i}\] is not finite"):
                    r.set_camera(bad)
        bad = copy_of(moved)
        bad.view[2] = float("nan")
        bad.position[0] = float("inf")  # the fields are looked at in the struct's order
        with pytest.raises(capi.PtError, match=r"camera position\[0\]"):
            r.set_camera(bad)
        st = r.stats()
        assert st.device_bytes == bytes_before and st.samples == 96 * 54 * 8 and r.setup_times().set_camera_calls == 0
        assert np.array_equal(bits(r.readback()), bits(want))  # nothing was cleared
        r.clear()
        assert np.array_equal(bits(render_two_calls(r)), bits(want))  # and the view is still A
        ok = copy_of(scene.camera)
        ok.lookAt[0] = float("nan")  # not read by the renderer
        r.set_camera(ok)
        assert np.array_equal(bits(render_two_calls(r)), bits(want))
    finally:
        r.free()
