"""Editing the materials of a live renderer (pt_set_materials): after the call the renderer gives what a renderer freshly created from
the scene with those materials gives, bit for bit — image (in one render call and in three), feature planes, noise planes, a threshold
round, the resolved and the filtered image — in all three arithmetic modes, with tables in LDS, from memory and with the grid walk.
The edited scenes are Scene.set_material on a loaded scene, or (for the oracle) scene texts with the MATERIAL blocks rewritten."""
import ctypes as C
import re

import numpy as np
import pytest

from cosc_4397_pathtracing_raytracing_project_amd import scenes

pytestmark = pytest.mark.gpu
f32 = np.float32
THRESHOLD, FRACTION = 0.02, 0.25


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    if isinstance(a, np.ndarray):
        return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    return a == b


# (text, res, debug_flags, the materials the edit touches: a diffuse wall, the light, the mirror, a diffuse one that becomes an emitter)
def cornell():      # 7 primitives: tables in LDS, record_form 2
    return scenes.cornell_scene_text(res=(96, 54)), (96, 54), 0, dict(wall=2, light=0, mirror=4, lamp=3)


def random45():     # tables from memory
    return scenes.random_scene_text(3, 45), (96, 64), 0, dict(wall=1, light=0, mirror=3, lamp=2)


def random349():    # the grid walk
    return scenes.random_scene_text(3, 349), (96, 64), 256, dict(wall=1, light=0, mirror=3, lamp=2)


# the edit M1, as text and as numbers: the words of the file and the float32 the setter takes are the same numbers
EDIT = dict(wall=dict(RGB=(".35", ".35", ".85")), light=dict(EMITTANCE=".75"), mirror=dict(REFL="0"), lamp=dict(EMITTANCE=".5"))


def edited_text(text, roles):
    """`text` with the lines of EDIT rewritten in the MATERIAL blocks of `roles`."""
    for role, lines in EDIT.items():
        for key, value in lines.items():
            new = " ".join(value) if isinstance(value, tuple) else value
            text, n = re.subn(r"(MATERIAL %d\n(?:(?!MATERIAL|CAMERA|OBJECT).*\n)*?%s\s+)[^\n]*" % (roles[role], key), lambda m: m.group(1) + new, text, count=1)
            assert n == 1, (role, key)
    return text


def edit_scene(scene, roles):
    """EDIT through Scene.set_material."""
    for role, lines in EDIT.items():
        m = scene.material(roles[role])
        for key, value in lines.items():
            if key == "RGB":
                m.color[:] = [float(f32(float(v))) for v in value]
            elif key == "EMITTANCE":
                m.emittance = float(f32(float(value)))
            else:
                m.hasReflective = float(f32(float(value)))
        scene.set_material(roles[role], m)


def sequence(r, calls):
    """12 iterations in `calls` render calls; then from a clear: render, features, the filter, two folds, one threshold round, and what can be read."""
    out = {}
    r.clear()
    for k in range(calls):
        r.render(1 + k * (12 // calls), 12 // calls)
    out["image12"] = r.readback()
    r.clear()
    r.render(1, 4)
    r.render_features(1, 4)
    out["denoise"] = r.denoise(4)
    r.noise_fold()
    r.render(5, 4)
    r.noise_fold()
    out["round"] = r.adaptive_round_threshold(9, 4, THRESHOLD, FRACTION)  # the worker exists, and must have received the table
    out["image"] = r.readback()
    for k, v in r.readback_noise().items():
        out["noise_" + k] = v
    for k, v in r.readback_features().items():
        out["feature_" + k] = v
    out["counts"] = r.readback_adaptive()
    out["resolved"] = r.resolve()
    return out


def check(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert same(got[k], want[k]), (what, k)


@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
@pytest.mark.parametrize("case", [cornell, random45, random349])
def test_edited_materials_equal_a_fresh_renderer(tmp_path, oracle, case, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    text, res, flags, roles = case()
    p0 = scenes.write_scene(text, str(tmp_path / "m0.txt"))
    p1 = scenes.write_scene(edited_text(text, roles), str(tmp_path / "m1.txt"))
    opts = dict(debug_flags=flags, arith=arith, iters_per_batch=4)
    s1 = capi.Scene(p0, res=res)
    edit_scene(s1, roles)
    loaded = capi.Scene(p1, res=res)
    assert [bytes(m) for m in s1.materials()] == [bytes(m) for m in loaded.materials()]  # the setter and the loader agree
    want = {}
    for name, scene in (("M0", capi.Scene(p0, res=res)), ("M1", s1)):
        fresh = capi.Renderer(scene, **opts)
        try:
            want[name] = sequence(fresh, 1)
            if name == "M1":
                want["M1 in three calls"] = sequence(fresh, 3)
                assert case is not cornell or fresh.stats().record_form == 2  # later batches read what the primary kernel left
        finally:
            fresh.free()
    check(want["M1 in three calls"], want["M1"], "one render call against three")
    assert not same(want["M0"]["image"], want["M1"]["image"]) and not same(want["M0"]["feature_albedo"], want["M1"]["feature_albedo"])
    assert want["M0"]["round"] != (0, 0) or want["M1"]["round"] != (0, 0)
    live = capi.Scene(p0, res=res)
    r = capi.Renderer(live, **opts)
    try:
        check(sequence(r, 3), want["M0"], "before any edit")  # a worker, folds and counts exist: all of it is forgotten
        before = r.stats().device_bytes
        edit_scene(live, roles)
        r.set_materials(live)
        assert not r.readback().any() and r.stats().samples == 0  # everything pt_clear does
        assert r.noise() == dict(sse=-1.0, groups=0, iterations=0) and not r.readback_adaptive().any()
        assert r.stats().device_bytes == before
        got = sequence(r, 1)
        check(got, want["M1"], "after set_materials(M1)")
        check(sequence(r, 3), want["M1"], "after set_materials(M1), in three calls")
        if arith == "exact":
            oracle.set_math_mode(oracle.PORTABLE)
            oracle.load_scene(p1, res=res)
            ref = oracle.render(1, 12, depth=8, variant=oracle.RETIRE, nthreads=16)
            assert np.array_equal(bits(got["image12"]), bits(ref))
        r.set_materials(live)  # unchanged materials change nothing in any result
        assert r.stats().device_bytes == before
        check(sequence(r, 1), want["M1"], "after a call with unchanged materials")
        r.set_materials(capi.Scene(p0, res=res))
        assert r.stats().device_bytes == before
        check(sequence(r, 1), want["M0"], "after set_materials(M0) again")
        t = r.set_materials_times()
        assert t.total_ms > 0 and t.upload_ms > 0 and t.rearm_ms > 0 and t.total_ms >= t.upload_ms + t.rearm_ms
        assert r.setup_times().set_camera_calls == 0 and r.set_geoms_times().total_ms == 0
    finally:
        r.free()


def test_history_lifetimes_across_set_materials(tmp_path):
    """K, VK and PK are kept byte for byte; C, VC and E become absent."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    text, res, _, roles = cornell()
    live = capi.Scene(scenes.write_scene(text, str(tmp_path / "m0.txt")), res=res)
    r = capi.Renderer(live)
    try:
        r.render(1, 4)
        r.render_features(1, 1)
        r.history_probe_keep(1, 4, 2)
        r.history_capture_ex(4, capi.HISTORY_MOMENTS)
        r.clear()
        r.render(5, 4)
        r.render_features(1, 1)
        r.history_reproject_ex(capi.HISTORY_MOMENTS)
        fresh, m = r.history_round(9, 2, 1000)
        assert m > 0
        K, Cur = r.readback_history()
        VK, VC = r.readback_history_variance()
        PK = r.readback_history_probe()[0]
        assert Cur.any() and VC.any() and r.readback_history_extra().any() and K.any() and VK.any() and PK.any()
        before = r.stats().device_bytes
        edit_scene(live, roles)
        r.set_materials(live)
        K1, C1 = r.readback_history()
        VK1, VC1 = r.readback_history_variance()
        assert same(K1, K) and same(VK1, VK) and same(r.readback_history_probe()[0], PK)
        assert not C1.any() and not VC1.any() and not r.readback_history_extra().any()
        assert r.stats().device_bytes == before
        with pytest.raises(capi.PtError, match="current plane is absent"):
            r.history_probe_check()
    finally:
        r.free()


def test_group_set_materials_equals_one_renderer(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    text, res, _, roles = cornell()
    p0 = scenes.write_scene(text, str(tmp_path / "m0.txt"))
    edited = capi.Scene(p0, res=res)
    edit_scene(edited, roles)

    def views(x):
        x.render(1, 4)
        x.render_features(1, 4)
        x.noise_fold()
        x.render(5, 4)
        x.noise_fold()
        rnd = x.adaptive_round_threshold(9, 4, THRESHOLD, FRACTION)
        return (rnd,) + ((x.gather(), x.gather_features()) if hasattr(x, "gather") else (x.readback(), x.readback_features()))

    r = capi.Renderer(capi.Scene(p0, res=res))
    try:
        r.render(1, 4)
        r.set_materials(edited)
        want = views(r)
    finally:
        r.free()
    g = capi.Group(capi.Scene(p0, res=res), [0, 0], transport="copy")
    try:
        g.render(1, 4)
        before = g.gather()
        bad = [capi.PtMaterial.from_buffer_copy(m) for m in edited.materials()]
        bad[3].specular_color[2] = float("nan")
        with pytest.raises(capi.PtError, match=r"pt_group_set_materials: specular_color of material 3 is not finite"):
            g.set_materials(bad)
        with pytest.raises(capi.PtError, match=r"pt_group_set_materials: 4 materials, but the renderer was created with 5"):
            g.set_materials(bad[:4])
        assert np.array_equal(bits(g.gather()), bits(before))  # nothing was cleared in either context
        g.set_materials(edited)
        assert not g.gather().any()
        got = views(g)
        assert got[0] == want[0] and want[0][1] > 0
        assert np.array_equal(bits(got[1]), bits(want[1]))
        for k in want[2]:
            assert same(got[2][k], want[2][k]), k
        for i in range(2):
            t = capi.PtSetMaterialsTimes()
            capi._check(capi.lib().pt_ctx_get_set_materials_times(g.context(i), C.byref(t)))
            assert t.total_ms > 0
    finally:
        g.free()


# ---- refusals: by phrase, in order, with nothing changed ------------------------------------------------------------------------
def test_refusals(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    L = capi.lib()
    text, res, _, roles = cornell()
    scene = capi.Scene(scenes.write_scene(text, str(tmp_path / "m0.txt")), res=res)
    capi.pt_free()
    for mats in (None, scene.desc.materials):  # no renderer comes before null materials
        assert L.pt_set_materials(mats, 5) != 0
        assert b"pt_set_materials: pt_init has not been called" in L.pt_last_error()
    assert L.pt_get_set_materials_times(C.byref(capi.PtSetMaterialsTimes())) != 0
    r = capi.Renderer(scene)
    try:
        r.render(1, 3)
        r.render(4, 5)
        want = r.readback()
        before = r.stats().device_bytes

        def refused(mats, n, phrase):
            assert L.pt_set_materials(mats, n) != 0
            msg = L.pt_last_error().decode()
            assert msg.startswith("pt_set_materials: ") and phrase in msg, msg

        arr = lambda ms: (capi.PtMaterial * len(ms))(*ms)
        bad = [capi.PtMaterial.from_buffer_copy(m) for m in scene.materials()]
        good = [capi.PtMaterial.from_buffer_copy(m) for m in bad]
        refused(None, 3, "null materials")                   # before the count
        bad[1].hasRefractive = float("nan")                   # the count comes before the words, and the first material is named,
        bad[3].color[0] = float("inf")                        # by the first of its words in the header's order
        bad[3].emittance = float("nan")
        refused(arr(bad), 4, "4 materials, but the renderer was created with 5; adding or removing materials needs pt_init")
        refused(arr(bad), 6, "6 materials")
        refused(arr(bad), 5, "hasRefractive of material 1 is not finite")
        bad[1].hasRefractive = 0.0
        refused(arr(bad), 5, "color of material 3 is not finite")
        bad[3].color[0] = good[3].color[0]
        refused(arr(bad), 5, "emittance of material 3 is not finite")
        bad[3].emittance = 0.0
        bad[4].specular_color[1] = float("-inf")
        refused(arr(bad), 5, "specular_color of material 4 is not finite")
        bad[4].specular_color[1] = good[4].specular_color[1]
        bad[0].hasReflective = float("nan")
        refused(arr(bad), 5, "hasReflective of material 0 is not finite")
        bad[0].hasReflective = 0.0
        bad[2].specular_exponent, bad[2].indexOfRefraction = float("nan"), float("inf")  # words the renderer does not read
        st = r.stats()
        assert st.device_bytes == before and st.samples == 96 * 54 * 8 and r.set_materials_times().total_ms == 0
        assert np.array_equal(bits(r.readback()), bits(want))  # nothing was cleared
        assert L.pt_set_materials(arr(bad), 5) == 0
        assert r.stats().device_bytes == before
        r.render(1, 3)
        r.render(4, 5)
        assert np.array_equal(bits(r.readback()), bits(want))  # the nine words are what they were
    finally:
        r.free()
