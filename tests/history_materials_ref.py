"""PT_HISTORY_MATERIALS of include/pt_amd.h restated in numpy: the recolour table (pt_history_recolor_host) and the lookup with the
recolour step (pt_history_reproject_materials_host) on top of tests/history_motion_ref.py's lookup, float32, one IEEE operation each in
the header's order, for the plain, the variance and the moments kind, with and without a motion table.  Also the inputs the host and
the GPU tests share."""
import numpy as np

import history_motion_ref as mot
import history_ref as href
from history_ref import bits, f32, surface  # noqa: F401  (bits: for the tests)

VARIANCE, MOMENTS, MOTION, FEEDBACK, MATERIALS = 1, 2, 4, 16, 32
ROW = 4
UNCHANGED, RECOLORED, NOTHING = 0, 1, 2
SHAPES = [(1, 1, 0), (67, 5, 0), (67, 5, 7)]  # (w, rows, row0): one pixel; no multiple of 4 or 64, more than one workgroup; row0 != 0


def material(color=(0.5, 0.5, 0.5), spec=(0.0, 0.0, 0.0), reflective=0.0, refractive=0.0, emittance=0.0, exponent=0.0, ior=0.0):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    m = capi.PtMaterial()
    m.color[:], m.specular_color[:] = [float(f32(x)) for x in color], [float(f32(x)) for x in spec]
    m.hasReflective, m.hasRefractive, m.emittance = float(f32(reflective)), float(f32(refractive)), float(f32(emittance))
    m.specular_exponent, m.indexOfRefraction = float(exponent), float(ior)
    return m


def _nine(m):
    return np.array(list(m.color) + list(m.specular_color) + [m.hasReflective, m.hasRefractive, m.emittance], f32)


def material_kind(k, c):
    """(mk, ratio float32 [3]) of one kept and one current material."""
    kw, cw = _nine(k), _nine(c)
    zero = np.zeros(3, f32)
    if np.array_equal(kw.view(np.uint32), cw.view(np.uint32)):
        return UNCHANGED, zero
    if not np.array_equal(kw[3:].view(np.uint32), cw[3:].view(np.uint32)) or kw[8] > 0 or kw[6] > 0:
        return NOTHING, zero
    with np.errstate(all="ignore"):
        if not (kw[:3] > 0).all() or not (cw[:3] >= 0).all():
            return NOTHING, zero
        r = (cw[:3] / kw[:3]).astype(f32)
    if not np.isfinite(r).all():
        return NOTHING, zero
    return RECOLORED, r


def recolor_table(kept, cur, geoms):
    """(table float32 [n, 4], kind uint8 [n]) for the n geoms, from two sequences of PtMaterial."""
    n = len(geoms)
    table, kind = np.zeros((n, ROW), f32), np.zeros(n, np.uint8)
    for g in range(n):
        m = geoms[g].materialid
        if 0 <= m < len(kept):
            kind[g], table[g, :3] = material_kind(kept[m], cur[m])
    return table, kind


def reproject_materials(cam, kept, feat, reject, recolor, rkind, w, rows, row0=0, flags=MATERIALS, kept_var=None, table=None, kind=None, **opts):
    """C [n, 4] (flags without a kind) or (C, VC): the lookup without the flag (with MOTION in `flags`: history_motion_ref's, else the
    same with every geom still), then kind 2 rejected and kind 1 scaled where the pixel was not rejected."""
    rkind = np.ascontiguousarray(rkind, np.uint8).reshape(-1)
    recolor = np.ascontiguousarray(recolor, f32).reshape(-1, ROW)
    ng = rkind.size
    if not flags & MOTION:
        table, kind = np.zeros((ng, mot.ROW), f32), np.zeros(ng, np.uint8)
    with_var = flags & (VARIANCE | MOMENTS)
    out = mot.reproject_motion(cam, kept, feat, reject, table, kind, w, rows, row0, flags=MOTION | with_var, kept_var=kept_var, **opts)
    C, VC = (out[0].copy(), out[1].copy()) if with_var else (out.copy(), None)
    # which pixels the lookup did not reject: the same lookup over a history of ones (Th = 1 exactly where a tap passed)
    ones = np.ascontiguousarray(kept, f32).reshape(3, -1, 4).copy()
    ones[0][ones[0][:, 3] > 0] = 1.0
    passed = mot.reproject_motion(cam, ones, feat, reject, table, kind, w, rows, row0, flags=MOTION, **dict(opts, cap=1.0))[:, 3] > 0
    hit, _, _, ids = surface(feat)
    inside = hit & (ids >= 1) & (ids <= ng)
    g = np.where(inside, ids - 1, 0)
    kd = np.where(inside, rkind[g], UNCHANGED)
    drop = kd == NOTHING
    C[drop] = 0
    scale = (kd == RECOLORED) & passed
    r = recolor[g][:, :3]
    with np.errstate(all="ignore"):
        C[scale, :3] = (C[:, :3] * r)[scale]
        if with_var:
            VC[drop] = 0
            VC[scale, :3] = ((VC[:, :3] * r).astype(f32) * r)[scale]
    return (C, VC) if with_var else C


def adversarial(w, rows, row0, seed=0):
    """history_motion_ref.adversarial's frame with edited materials in it: ids 1 and 4 are unchanged, 2 and 5 recoloured (5 with a
    channel whose factor is -0, 2 also moved), 3 is the mirror in `reject`, 6 carries nothing.
    Returns (cam, kept, feat, reject, table, kind, kept_var, recolor, rkind)."""
    cam, kept, feat, reject, _, table, kind, kept_var = mot.adversarial(w, rows, row0, seed)
    rkind = np.array([UNCHANGED, RECOLORED, RECOLORED, UNCHANGED, RECOLORED, NOTHING], np.uint8)
    recolor = np.zeros((href.NUM_GEOMS, ROW), f32)
    recolor[1, :3] = (0.5, 2.25, 1.0 / 3.0)
    recolor[2, :3] = (3.0, 0.125, 7.0)
    recolor[4, :3] = (-0.0, 1e-39, 1.7)  # -0: a rejected pixel must stay +0; a denormal factor is carried as computed
    rng = np.random.default_rng(5 + 100 * w + 10 * rows + row0)
    recolor[0], recolor[5] = rng.random(ROW, dtype=f32), rng.random(ROW, dtype=f32)  # rows of kinds 0 and 2 are never read
    return cam, kept, feat, reject, table, kind, kept_var, recolor, rkind


KINDS = {"plain": MATERIALS, "variance": MATERIALS | VARIANCE, "moments": MATERIALS | MOMENTS}


# ---- the simulations of tests/test_history_materials_sim.py: cornell 96 x 54, depth 8, the sphere mirror as in cornell.txt, the camera
# still, 8 views of 4 spp (view f renders iterations 4 f + 1 ...), the moments kind; before view 4 a material is edited; scored against
# 1024 spp of the last view's scene ------------------------------------------------------------------------------------------------
EDIT_VIEW = 4
SIM_WALL, SIM_WALL_GEOM, SIM_LIGHT = 2, 4, 0   # the red material (the left wall alone has it), the light's
SIM_EDITS = {"recolour": (SIM_WALL, "RGB", ".35 .35 .85"), "dimmed": (SIM_LIGHT, "EMITTANCE", ".75")}
PROBE_SCAN = [(r, g) for r in (0, 1) for g in (0.25, 1.0, 2.0, 4.0)]  # (radius, gain); (0, 0.25) are the defaults


def edited_text(text, material, key, value):
    """`text` with the line `key` of MATERIAL block `material` rewritten."""
    import re
    text, n = re.subn(r"(MATERIAL %d\n(?:(?!MATERIAL|CAMERA|OBJECT).*\n)*?%s\s+)[^\n]*" % (material, key), lambda m: m.group(1) + value, text, count=1)
    assert n == 1, (material, key)
    return text


def sim_scene_paths(directory, which):
    """(the scene before the edit, the scene after it)."""
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    text = scenes.cornell_scene_text(res=href.RES, depth=8)
    return (scenes.write_scene(text, str(directory / f"{which}_before.txt")),
            scenes.write_scene(edited_text(text, *SIM_EDITS[which]), str(directory / f"{which}_after.txt")))


def copy_materials(scene):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    return [capi.PtMaterial.from_buffer_copy(m) for m in scene.materials()]


def run_sim(views, replays, reject, w, h, spp=href.SPP, flagged=True, probes=None):
    """The command line's --orbit --orbit-still --reproject [--history-probe] sequence with the moments kind through the library's host
    functions.  views: (camera, geoms, materials, S, feature planes) per view; replays[f]: view f - 1's iterations rendered in view f's
    scene (whole frame).  flagged: the lookup passes PT_HISTORY_MATERIALS; probes: None, or (radius, gain).  Returns per view
    dict(blend, C, L, changed, skipped)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    out = []
    K = VK = PK = kept_cam = kept_mats = probe_mats = None
    for f, (cam, geoms, mats, S, feat) in enumerate(views):
        C = VC = L = None
        changed = skipped = 0
        if K is not None:
            recolor, rkind = capi.history_recolor_host(kept_mats, mats, geoms)
            if flagged and rkind.any():
                C, VC = capi.history_reproject_materials_host(kept_cam, K, feat, reject, recolor, rkind, w, h, flags=MATERIALS | MOMENTS, kept_var=VK)
            else:
                C, VC = capi.history_reproject_moments_host(kept_cam, K, feat, reject, VK, w, h)
            if probes is not None:
                phase = (f - 1) % 9
                lst = capi.history_probe_list_host(w, h, phase)
                moved = (capi.history_recolor_host(probe_mats, mats, geoms)[1] != 0).astype(np.uint8)
                L, changed, skipped = capi.history_probe_gradient_host(PK, replays[f][lst], feat, w, h, phase, moved)
                C = capi.history_probe_apply_host(C, L, feat, w, h, phase, moved, radius=probes[0] or -1, gain=probes[1])
        if probes is not None:
            PK, probe_mats = capi.history_probe_keep_host(S, feat, w, h, f % 9), mats
        out.append(dict(blend=capi.history_blend_host(S, spp, C), C=C, L=L, changed=changed, skipped=skipped))
        K, VK, kept_cam, kept_mats = capi.history_capture_host(S, feat, spp, C), capi.history_capture_moments_host(S, spp, C, VC), cam, mats
    return out


# what tests/test_history_materials_sim.py prints (the exact build reproduces them on the device: tests/test_gpu_history_materials_sim.py)
# recolour: the wall's pixels, of those carried by the flagged lookup, MSE over the wall of the raw frame, the plain blend and the flagged
# blend, and the same three over the rest of the frame (the step touches no pixel off the wall)
SIM_RECOLOUR = dict(pixels=526, carried=526, wall_raw=0.00784753569, wall_plain=0.00299608258, wall_flagged=0.0012503966, rest_raw=0.0069672087,
                    rest_plain=0.00133956303, rest_flagged=0.00133956303)
# dimmed light: the frame's MSE without probes and per (radius, gain); (changed, skipped) per view with probes.  Without next-event
# estimation few of a view's 4 samples per pixel end on the small light — most of the box's light is the sky's, through the open front —
# so 53 of the 266 replayed probes change at the edit, with L up to 0.5; every other view replays to exactly its kept sums
SIM_DIMMED = {"none": 0.000874187694, "r0g0.25": 0.000866135018, "r0g1": 0.000845303455, "r0g2": 0.000860684771, "r0g4": 0.000893987561,
              "r1g0.25": 0.000847553011, "r1g1": 0.000787112907, "r1g2": 0.000923977117, "r1g4": 0.00101446477}
SIM_DIMMED_COUNTS = [(0, 287), (0, 304), (0, 304), (53, 310), (0, 320), (0, 320), (0, 304)]
