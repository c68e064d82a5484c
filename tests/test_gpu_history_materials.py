"""The history across a material edit on the device (PT_HISTORY_MATERIALS): k_history_reproject_materials against the host functions,
bit for bit, through the stage (exact, fma and fast) and through a renderer whose wall pt_set_materials recoloured and whose light it
dimmed, once with a moved sphere and PT_HISTORY_MOTION beside; the call with nothing edited against the call without the flag; the
refusals of the flag word."""
import ctypes as C

import numpy as np
import pytest

import history_materials_ref as ref
import history_motion_ref as mot
import history_ref as href
from history_ref import bits, f32

pytestmark = pytest.mark.gpu
RES = href.RES
W, H = RES
SPP = href.SPP
VAR, MOM, MOTION, FB, MATERIALS = ref.VARIANCE, ref.MOMENTS, ref.MOTION, ref.FEEDBACK, ref.MATERIALS
LIGHT, WALL = 0, 2  # the materials edited: the light's (geom 0) and the red one, which the left wall (geom 4) and the sphere (geom 6) share
WALL_GEOM, LIGHT_GEOM = 4, 0


def same(got, want, what=""):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


@pytest.fixture(scope="module")
def sphere_paths(tmp_path_factory):
    return mot.sim_scene_paths(tmp_path_factory.mktemp("gpu_history_materials"))  # cornell 96 x 54, depth 8, the sphere diffuse


# ---- the kernels on the arrays of the host tests ----------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
@pytest.mark.parametrize("motion", [0, MOTION])
@pytest.mark.parametrize("kind_name", sorted(ref.KINDS))
@pytest.mark.parametrize("w,rows,row0", ref.SHAPES)
def test_stage_equals_host(scene_dir, w, rows, row0, kind_name, motion, arith):
    """One pixel; 67 x 5, no multiple of 4 or 64 and two workgroups with a ragged last one, also at row0 != 0; unchanged, recoloured (a -0
    and a denormal factor among them) and kind-2 geoms in one frame, with and without moved ones."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    cam, kept, feat, reject, table, kind, vk, recolor, rkind = ref.adversarial(w, rows, row0)
    flags = ref.KINDS[kind_name] | motion
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(32, 24)), arith=arith)
    try:
        for name in ("defaults", "custom", "keep_view_dependent"):
            args = (cam.to_capi(), kept, feat, reject, recolor, rkind, w, rows, row0)
            kw = dict(flags=flags, kept_var=vk if flags & 3 else None, table=table if motion else None, kind=kind if motion else None, **href.OPTION_SETS[name])
            got, want = capi.stage_history_reproject_materials(*args, **kw), capi.history_reproject_materials_host(*args, **kw)
            if flags & 3:
                same(got[0], want[0], name), same(got[1], want[1], name)
            else:
                same(got, want, name)
    finally:
        r.free()


# ---- a renderer whose materials were edited: the planes on the device against the host functions on what it read back -----------------
def one_view(r, first, flags):
    if flags & VAR:  # the variance kind wants two folds
        r.render(first, SPP // 2)
        r.noise_fold()
        r.render(first + SPP // 2, SPP - SPP // 2)
        r.noise_fold()
    else:
        r.render(first, SPP)
    r.render_features(1, 1)


def planes(r, flags):
    kept, cur = r.readback_history()
    vk, vc = r.readback_history_variance() if flags & 3 else (None, None)
    return kept, cur, vk, vc


def copy_materials(scene):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    return [capi.PtMaterial.from_buffer_copy(m) for m in scene.materials()]


def edit(scene):
    """The red wall becomes blue, the light is dimmed."""
    m = scene.material(WALL)
    m.color[:] = [float(f32(x)) for x in (0.35, 0.35, 0.85)]
    scene.set_material(WALL, m)
    m = scene.material(LIGHT)
    m.emittance = float(f32(0.75))
    scene.set_material(LIGHT, m)


@pytest.mark.parametrize("kind_name,motion,row0,rows", [("plain", 0, 0, H), ("variance", 0, 10, 31), ("moments", 0, 0, H), ("moments", MOTION, 10, 31)])
def test_renderer_lookup_equals_host(sphere_paths, kind_name, motion, row0, rows):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    flags = ref.KINDS[kind_name] | motion
    kflags = flags & 3
    scene = capi.Scene(sphere_paths[0], res=RES)
    kept_geoms, kept_materials = mot.copy_geoms(scene), copy_materials(scene)
    ng = len(kept_geoms)
    r = capi.Renderer(scene, pixel_begin=row0 * W, pixel_count=rows * W, arith="fast")  # the history does not depend on the build
    try:
        one_view(r, 1, flags)
        r.history_capture_ex(SPP, kflags)
        kept_cam = scene.camera
        # nothing edited: the call with the flag is the call without it, and allocates nothing
        r.history_reproject_ex(kflags | motion)
        _, plain_C, _, plain_VC = planes(r, flags)
        before = r.stats().device_bytes
        r.history_reproject_ex(flags)
        _, C, _, VC = planes(r, flags)
        same(C, plain_C), same(VC if kflags else C, plain_VC if kflags else C)
        assert r.stats().device_bytes == before and (C[:, 3] > 0).any()
        # the edit (and, with MOTION, a move of the sphere); the camera stays
        edit(scene)
        r.set_materials(scene)
        if motion:
            trs = scene.geom_trs(mot.SPHERE)
            trs[0] += f32(0.75)
            scene.set_geom_trs(mot.SPHERE, trs)
            r.set_geoms(scene)
        grown = 97 * ng if motion else 0
        one_view(r, SPP + 1, flags)
        feat = r.readback_feature_planes()
        reject = capi.reject_geoms(scene)
        kept, _, vk, _ = planes(r, flags)
        r.history_reproject_ex(flags)
        assert r.stats().device_bytes - before == 17 * ng + grown  # 16 + 1 bytes per geom, by the first call that found a material changed
        _, C, _, VC = planes(r, flags)
        recolor, rkind = capi.history_recolor_host(kept_materials, copy_materials(scene), scene)
        want_kind = [{WALL: ref.RECOLORED, LIGHT: ref.NOTHING}.get(g.materialid, ref.UNCHANGED) for g in kept_geoms]
        assert list(rkind) == want_kind and want_kind[WALL_GEOM] == want_kind[mot.SPHERE] == ref.RECOLORED and want_kind[LIGHT_GEOM] == ref.NOTHING
        same(recolor[mot.SPHERE], recolor[WALL_GEOM])  # two geoms sharing a material
        table, kind = capi.history_motion_host(kept_geoms, mot.copy_geoms(scene)) if motion else (None, None)
        want = capi.history_reproject_materials_host(kept_cam, kept, feat, reject, recolor, rkind, W, rows, row0, flags=flags, kept_var=vk, table=table, kind=kind)
        if kflags:
            same(C, want[0], "C"), same(VC, want[1], "VC")
        else:
            same(C, want, "C")
        ids = href.surface(feat)[3]
        wall, light = (ids == WALL_GEOM + 1) | (ids == mot.SPHERE + 1), ids == LIGHT_GEOM + 1
        assert wall.sum() > 100 and (C[wall, 3] > 0).sum() > wall.sum() // 2 and not C[light].any()
        assert row0 > 0 or light.sum() > 10  # (the light is in the frame's first rows)
        # without the flag the lookup knows nothing of the edit: the wall carries its old colour, the light its old radiance
        r.history_reproject_ex(kflags | motion)
        _, old_C, _, old_VC = planes(r, flags)
        carried = wall & (C[:, 3] > 0)
        same(C[carried, :3], old_C[carried, :3] * recolor[WALL_GEOM, :3], "the wall's history, scaled")
        same(C[:, 3], np.where(light, f32(0), old_C[:, 3]), "Th")
        assert row0 > 0 or (old_C[light, 3] > 0).any()
        same(old_C[~wall & ~light], C[~wall & ~light], "the pixels of unchanged geoms")
        if kflags:
            same(VC[carried, :3], (old_VC[carried, :3] * recolor[WALL_GEOM, :3]).astype(f32) * recolor[WALL_GEOM, :3], "the wall's variance, scaled twice")
            same(VC[carried, 3], old_VC[carried, 3])
        r.history_reproject_ex(flags)  # the same kept materials again: nothing is uploaded, the same planes
        assert r.stats().device_bytes - before == 17 * ng + grown
        same(planes(r, flags)[1], C)
        # a capture keeps the materials as they are now: from then on nothing is edited
        r.history_capture_ex(SPP, kflags)
        r.history_reproject_ex(kflags | motion)
        plain_C = planes(r, flags)[1]
        r.history_reproject_ex(flags)
        same(planes(r, flags)[1], plain_C, "after a capture with the edited materials")
        assert row0 > 0 or (plain_C[light, 3] > 0).any()  # the light's pixels carry history again
    finally:
        r.free()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_flag_word(sphere_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    L = capi.lib()
    scene = capi.Scene(sphere_paths[0], res=RES)

    def refused(rc, *phrases):
        assert rc != 0
        msg = L.pt_last_error().decode()
        for ph in phrases:
            assert ph in msg, (ph, msg)

    who = "pt_history_reproject_ex"
    r = capi.Renderer(scene, pixel_begin=10, pixel_count=W * 3)  # the flag word comes before the ragged tile
    try:
        before = r.stats().device_bytes
        refused(L.pt_history_reproject_ex(None, MATERIALS | 8), who, "undefined flag bit(s) 0x8", "PT_HISTORY_MATERIALS")
        refused(L.pt_history_reproject_ex(None, MATERIALS | VAR | MOM), who, "exclude each other")
        for flags in (MATERIALS | MOM | FB, MATERIALS | MOM | FB | MOTION):
            refused(L.pt_history_reproject_ex(None, flags), who, "PT_HISTORY_MATERIALS is not built beside PT_HISTORY_FEEDBACK")
        for flags in (MATERIALS, MATERIALS | MOM, MATERIALS | MOM | FB):  # the capture does not define it
            refused(L.pt_history_capture_ex(C.c_float(-1.0), flags), "pt_history_capture_ex", "undefined flag bit(s) 0x20")
        for flags in (MATERIALS, MATERIALS | VAR, MATERIALS | MOM, MATERIALS | MOTION):
            refused(L.pt_history_reproject_ex(None, flags), who, "whole contiguous image rows")
        assert r.stats().device_bytes == before
    finally:
        r.free()
    r = capi.Renderer(scene)
    try:
        before = r.stats().device_bytes
        for flags in (MATERIALS, MATERIALS | VAR, MATERIALS | MOM):  # the flag with nothing captured: the existing message
            refused(L.pt_history_reproject_ex(None, flags), who, "nothing has been captured")
        assert r.stats().device_bytes == before
    finally:
        r.free()
    g = capi.Group(scene, [0, 0], transport="copy")
    try:
        g.render(1, SPP)
        g.render_features(1, 1)
        with pytest.raises(capi.PtError, match="pt_group_history_reproject_ex: PT_HISTORY_MATERIALS is not built for a group"):
            g.history_reproject_ex(MATERIALS | MOM)
        with pytest.raises(capi.PtError, match="pt_group_history_capture_ex: undefined flag bit"):
            g.history_capture_ex(SPP, MATERIALS | MOM)
    finally:
        g.free()


def test_the_adaptive_capture_keeps_the_materials_too(sphere_paths):
    """pt_history_capture_adaptive is a capture like the others: a renderer whose only capture it was looks up with the flag against the
    materials it had then, and a second such capture after the edit keeps the edited ones (nothing is scaled twice)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(sphere_paths[0], res=RES)
    kept_materials, kept_cam = copy_materials(scene), scene.camera
    flags = MATERIALS | VAR
    r = capi.Renderer(scene, arith="fast")
    try:
        r.render_features(1, 1)
        r.history_render_threshold(1, 12, 0.25, 0.5, 2, 3)
        r.history_capture_adaptive()  # the renderer's first capture of any kind
        edit(scene)
        r.set_materials(scene)
        r.render_features(1, 1)
        feat = r.readback_feature_planes()
        kept, _, vk, _ = planes(r, flags)
        r.history_reproject_ex(flags)
        _, C, _, VC = planes(r, flags)
        recolor, rkind = capi.history_recolor_host(kept_materials, copy_materials(scene), scene)
        assert rkind[WALL_GEOM] == ref.RECOLORED and rkind[LIGHT_GEOM] == ref.NOTHING
        want = capi.history_reproject_materials_host(kept_cam, kept, feat, capi.reject_geoms(scene), recolor, rkind, W, H, 0, flags=flags, kept_var=vk)
        same(C, want[0], "C"), same(VC, want[1], "VC")
        r.history_reproject_ex(VAR)
        plain_C = planes(r, flags)[1]
        wall = (href.surface(feat)[3] == WALL_GEOM + 1) & (C[:, 3] > 0)
        assert wall.sum() > 100 and not np.array_equal(bits(C[wall, :3]), bits(plain_C[wall, :3]))  # the flag was not ignored
        # the second view's capture keeps the edited materials: from then on the flag changes nothing
        r.history_reproject_ex(flags)
        r.history_render_threshold(101, 12, 0.25, 0.5, 2, 3)
        r.history_capture_adaptive()
        r.clear()
        r.render_features(1, 1)
        r.history_reproject_ex(VAR)
        plain_C, plain_VC = planes(r, flags)[1::2]
        r.history_reproject_ex(flags)
        same(planes(r, flags)[1], plain_C, "C after a second adaptive capture"), same(planes(r, flags)[3], plain_VC, "VC")
    finally:
        r.free()
