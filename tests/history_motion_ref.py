"""PT_HISTORY_MOTION of include/pt_amd.h restated in numpy: the motion table in float64 operations rounded to float32 once
(pt_history_motion_host), and the lookup with the motion step in float32 operations, one IEEE operation each in the header's order
(pt_history_reproject_motion_host), for the plain, the variance and the moments kind.  Also the inputs the host and the GPU tests
share, and the digits of the simulation (tests/test_history_motion_sim.py)."""
import numpy as np

import history_ref as href
from history_ref import bits, dot3, f32, surface  # noqa: F401  (bits: for the tests)

VARIANCE, MOMENTS, MOTION = 1, 2, 4
ROW = 24
STILL, MOVED, NOTHING = 0, 1, 2


def _mat(m):
    """A PtGeom matrix (16 floats, column-major m[c*4+r]) as float64 [r][c]."""
    return np.array(list(m), f32).astype(np.float64).reshape(4, 4).T


def _words(g):
    return np.array(list(g.transform) + list(g.inverseTransform) + list(g.invTranspose), f32).view(np.uint32)


def motion_table(kept, cur):
    """(table float32 [n, 24], kind uint8 [n]) from two sequences of PtGeom."""
    n = len(kept)
    table, kind = np.zeros((n, ROW), f32), np.zeros(n, np.uint8)
    with np.errstate(all="ignore"):
        for g in range(n):
            A_k, B_c = _mat(kept[g].transform), _mat(cur[g].inverseTransform)
            IT_k, A_c = _mat(kept[g].invTranspose), _mat(cur[g].transform)
            for r in range(3):
                for c in range(4):
                    table[g, r * 4 + c] = f32(((A_k[r, 0] * B_c[0, c] + A_k[r, 1] * B_c[1, c]) + A_k[r, 2] * B_c[2, c]) + A_k[r, 3] * B_c[3, c])
                for c in range(3):
                    table[g, 12 + r * 3 + c] = f32((IT_k[r, 0] * A_c[c, 0] + IT_k[r, 1] * A_c[c, 1]) + IT_k[r, 2] * A_c[c, 2])
            if np.array_equal(_words(kept[g]), _words(cur[g])):
                kind[g] = STILL
            elif kept[g].type == 2 or cur[g].type == 2 or not np.isfinite(table[g, :21]).all():
                kind[g] = NOTHING
            else:
                kind[g] = MOVED
    return table, kind


def reproject_motion(cam, kept, feat, reject, table, kind, w, rows, row0=0, flags=MOTION, kept_var=None, stats=None, **opts):
    """C [n, 4] (flags without a kind) or (C, VC): history_ref.reproject / reproject_variance / reproject_moments with the motion step
    after the first rejections.  stats: receives sx, sy, dz, wsum, moved per pixel."""
    cap, min_dot, plane_tol, keep = href.resolve_options(**opts)
    W, H = int(cam.resolution[0]), int(cam.resolution[1])
    assert W == w
    pos, view, up, right = (np.array(list(v), f32) for v in (cam.position, cam.view, cam.up, cam.right))
    plx, ply = f32(cam.pixelLength[0]), f32(cam.pixelLength[1])
    hw, hh = f32(W) * f32(0.5), f32(H) * f32(0.5)
    K = np.ascontiguousarray(kept, f32).reshape(3, -1, 4)
    with_var = flags & (VARIANCE | MOMENTS)
    nv = 4 if flags & MOMENTS else 3
    VK = None if not with_var else np.ascontiguousarray(kept_var, f32).reshape(-1, 4)
    npix = w * rows
    hit, n, p, ids = surface(feat)
    reject = np.ascontiguousarray(reject, np.uint8).reshape(-1)
    table = np.ascontiguousarray(table, f32).reshape(-1, ROW)
    kind = np.ascontiguousarray(kind, np.uint8).reshape(-1)
    ok = hit.copy()
    inside = (ids >= 1) & (ids <= kind.size)
    if not keep:
        listed = np.zeros(npix, bool)
        listed[inside] = reject[ids[inside] - 1] != 0
        ok &= inside & ~listed
    with np.errstate(all="ignore"):
        # the motion step: kind per pixel (an id outside 1 .. num_geoms is still), p' and n' for the moved ones
        g = np.where(inside, ids - 1, 0)
        kd = np.where(inside, kind[g], STILL)
        ok &= kd != NOTHING
        moved = ok & (kd == MOVED)
        D = table[g]
        q3 = np.stack([((D[:, 4 * r] * p[:, 0] + D[:, 4 * r + 1] * p[:, 1]) + D[:, 4 * r + 2] * p[:, 2]) + D[:, 4 * r + 3] for r in range(3)], axis=1)
        m = np.stack([dot3(D[:, 12 + 3 * r], D[:, 13 + 3 * r], D[:, 14 + 3 * r], n[:, 0], n[:, 1], n[:, 2]) for r in range(3)], axis=1)
        l = dot3(m[:, 0], m[:, 1], m[:, 2], m[:, 0], m[:, 1], m[:, 2])
        ok &= ~(moved & ~(l > 0))
        rr = np.sqrt(l)
        p = np.where(moved[:, None], q3, p).astype(f32)
        n = np.where(moved[:, None], m / rr[:, None], n).astype(f32)

        v = p - pos
        dz = dot3(v[:, 0], v[:, 1], v[:, 2], view[0], view[1], view[2])
        ok &= dz > 0
        sx = hw - dot3(v[:, 0], v[:, 1], v[:, 2], right[0], right[1], right[2]) / (dz * plx)
        sy = hh - dot3(v[:, 0], v[:, 1], v[:, 2], up[0], up[1], up[2]) / (dz * ply)
        fx, fy = np.floor(sx), np.floor(sy)
        ok &= (fx >= -1) & (fx <= f32(W - 1)) & (fy >= -1) & (fy <= f32(H - 1))
        ax, ay = sx - fx, sy - fy
        ix = np.where(ok, fx, 0).astype(np.int64)
        iy = np.where(ok, fy, 0).astype(np.int64) - row0
        tol = plane_tol * dz
        acc, vacc = np.zeros((npix, 3), f32), np.zeros((npix, 4), f32)
        tacc, wsum = np.zeros(npix, f32), np.zeros(npix, f32)
        for j in (0, 1):
            for i in (0, 1):
                qx, qr = ix + i, iy + j
                take = ok & (qx >= 0) & (qx < w) & (qr >= 0) & (qr < rows)
                q = np.where(take, qr * w + qx, 0)
                k0, k1, k2 = K[0][q], K[1][q], K[2][q]
                take &= k0[:, 3] > 0
                take &= np.ascontiguousarray(k1[:, 3]).view(np.int32) == ids
                if min_dot >= 0:
                    take &= ~(dot3(n[:, 0], n[:, 1], n[:, 2], k2[:, 0], k2[:, 1], k2[:, 2]) < min_dot)
                if plane_tol >= 0:
                    e = dot3(n[:, 0], n[:, 1], n[:, 2], k1[:, 0] - p[:, 0], k1[:, 1] - p[:, 1], k1[:, 2] - p[:, 2])
                    take &= ~(np.abs(e) > tol)
                b = (ax if i else f32(1) - ax) * (ay if j else f32(1) - ay)
                for k in range(3):
                    acc[:, k] = np.where(take, acc[:, k] + b * k0[:, k], acc[:, k])
                tacc = np.where(take, tacc + b * k0[:, 3], tacc)
                if with_var:
                    vk = VK[q]
                    for k in range(nv):
                        vacc[:, k] = np.where(take, vacc[:, k] + b * vk[:, k], vacc[:, k])
                wsum = np.where(take, wsum + b, wsum)
        ok &= wsum >= href.MIN_WEIGHT
        h = acc / wsum[:, None]
        vh = vacc / wsum[:, None]
        t = tacc / wsum
        th = np.where(t < cap, t, cap)
    if stats is not None:
        stats.update(sx=sx, sy=sy, dz=dz, wsum=wsum, moved=moved)
    C, VC = np.zeros((npix, 4), f32), np.zeros((npix, 4), f32)
    C[ok, :3], C[ok, 3] = h[ok], th[ok]
    VC[ok, :nv] = vh[ok, :nv]
    return (C, VC) if with_var else C


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def geom(trs, kind=1, material=1):
    """A PtGeom placed by the loader's code (pt_build_transform)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    g = capi.PtGeom()
    g.type, g.materialid = kind, material
    t, inv, it = capi.build_transform(trs)
    g.transform[:], g.inverseTransform[:], g.invTranspose[:] = t.tolist(), inv.tolist(), it.tolist()
    return g


def copy_geoms(scene):
    """The scene's geoms as copies of their own: Scene.geoms() points into memory that pt_scene_free gives back."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    return [capi.PtGeom.from_buffer_copy(g) for g in scene.geoms()]


def triangle(vertices):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    g = capi.PtGeom()
    g.type, g.materialid = 2, 1
    g.transform[:9] = [float(x) for x in vertices]
    return g


def mixed_geoms():
    """(kept, cur) for history_ref.NUM_GEOMS geoms: still, translated, rotated and scaled (non-uniform), a changed triangle (kind 2),
    a singular current transform (kind 2: the loader's inverse of scale 0 is not finite), still."""
    kept = [geom((0, 0, 0, 0, 0, 0, 1, 1, 1)), geom((1, 2, 3, 0, 0, 0, 1, 1, 1)), geom((0.5, 0, 2, 10, 20, 30, 1, 2, 0.5)),
            triangle((0, 0, 0, 1, 0, 0, 0, 1, 0)), geom((0, 1, 0, 0, 0, 0, 1, 1, 1)), geom((3, 3, 3, 45, 0, 0, 2, 2, 2))]
    cur = [geom((0, 0, 0, 0, 0, 0, 1, 1, 1)), geom((1.5, 2, 2.75, 0, 0, 0, 1, 1, 1)), geom((0.25, 0.5, 2, 25, 5, 60, 1.5, 2, 0.25)),
           triangle((0, 0, 0.5, 1, 0, 0.5, 0, 1, 0.5)), geom((0, 1, 0, 0, 0, 0, 1, 0, 1)), geom((3, 3, 3, 45, 0, 0, 2, 2, 2))]
    return kept, cur


def adversarial(w, rows, row0, seed=0):
    """history_ref.adversarial's frame with moved, still and kind-2 geoms in it: ids 1 and 6 are still, 2 is translated by a quarter
    pixel's worth along x and 1/8 in depth, 3 (a mirror in `reject`) and 5 are rotated about the view axis with a non-uniform scale
    of the normal, 4 carries nothing.  Returns (cam, kept, feat, reject, plant, table, kind, kept_var)."""
    cam, kept, feat, reject, plant = href.adversarial(w, rows, row0, seed)
    rng = np.random.default_rng(77 + 1000 * seed + 100 * w + 10 * rows + row0)
    table = np.zeros((href.NUM_GEOMS, ROW), f32)
    kind = np.array([STILL, MOVED, MOVED, NOTHING, MOVED, STILL], np.uint8)
    eye3 = np.eye(3, dtype=f32)
    for g in range(href.NUM_GEOMS):
        table[g, :12] = np.concatenate([eye3, np.zeros((3, 1), f32)], axis=1).ravel()
        table[g, 12:21] = eye3.ravel()
    table[1, 3], table[1, 11] = f32(0.0625), f32(0.125)
    c, s = f32(np.cos(0.05)), f32(np.sin(0.05))
    for g in (2, 4):
        table[g, :12] = np.array([[c, -s, 0, 0.03125], [s, c, 0, -0.015625], [0, 0, 1, 0]], f32).ravel()
        table[g, 12:21] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 0.5]], f32).ravel()
    table[0] = rng.random(ROW, dtype=f32)  # a still geom's row is never read
    kept_var = rng.random((w * rows, 4), dtype=f32)
    return cam, kept, feat, reject, plant, table, kind, kept_var


KINDS = {"plain": MOTION, "variance": MOTION | VARIANCE, "moments": MOTION | MOMENTS}

# ---- the simulation of tests/test_history_motion_sim.py: cornell 96 x 54, depth 8, the sphere diffuse (material 2), the camera still,
# the sphere's TRANS x from -2.5 in steps of 0.5 over 8 views, 4 spp per view, scored against 1024 spp at the last view ----------------
SPHERE, SPHERE_MATERIAL, SPHERE_X0, SPHERE_STEP = 6, 2, -2.5, 0.5


def sphere_objects(frame, step=SPHERE_STEP):
    return {SPHERE: dict(trans=(SPHERE_X0 + step * frame, 4, -1), material=SPHERE_MATERIAL)}


def sim_scene_paths(directory, step=SPHERE_STEP, frames=href.FRAMES):
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    return [scenes.write_scene(scenes.cornell_scene_text(res=href.RES, depth=8, objects=sphere_objects(f, step)), str(directory / f"sphere_move{f}.txt"))
            for f in range(frames)]


def run_sequence(views, fns, spp=href.SPP, motion=True):
    """The command line's --orbit --reproject --move sequence with the moments kind over `views`, a list of (camera, geoms, S, feature
    planes): from the second view on the history is looked up — with the motion table of the kept and the current geoms, or (motion
    False) as if the world stood still — then the view is resolved, then captured with its moments.  fns: capture, capture_moments,
    blend, motion_table, reproject_motion, reproject_moments (the host functions, or this module's).  Returns per view (blend, C, VC)."""
    out = []
    K = VK = kept_cam = kept_geoms = None
    for cam, geoms, S, feat in views:
        if K is None:
            C = VC = None
        elif motion:
            table, kind = fns["motion_table"](kept_geoms, geoms)
            C, VC = fns["reproject_motion"](kept_cam, K, feat, VK, table, kind)
        else:
            C, VC = fns["reproject_moments"](kept_cam, K, feat, VK)
        out.append((fns["blend"](S, spp, C), C, VC))
        K, VK, kept_cam, kept_geoms = fns["capture"](S, feat, spp, C), fns["capture_moments"](S, spp, C, VC), cam, geoms
    return out


def host_functions(reject, w, h):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    return dict(capture=lambda S, feat, spp, C: capi.history_capture_host(S, feat, spp, C),
                capture_moments=lambda S, spp, C, VC: capi.history_capture_moments_host(S, spp, C, VC),
                blend=lambda S, spp, C: capi.history_blend_host(S, spp, C),
                motion_table=capi.history_motion_host,
                reproject_motion=lambda cam, K, feat, VK, table, kind: capi.history_reproject_motion_host(cam, K, feat, reject, table, kind, w, h,
                                                                                                         flags=MOTION | MOMENTS, kept_var=VK),
                reproject_moments=lambda cam, K, feat, VK: capi.history_reproject_moments_host(cam, K, feat, reject, VK, w, h))


def ref_functions(reject, w, h):
    import history_moments_ref as mref
    return dict(capture=href.capture, capture_moments=mref.capture_moments, blend=href.blend, motion_table=motion_table,
                reproject_motion=lambda cam, K, feat, VK, table, kind: reproject_motion(cam, K, feat, reject, table, kind, w, h,
                                                                                       flags=MOTION | MOMENTS, kept_var=VK),
                reproject_moments=lambda cam, K, feat, VK: mref.reproject_moments(cam, K, feat, reject, VK, w, h))


def sphere_scores(out, feat, S, truth, spp=href.SPP):
    """Of the last view: the sphere's pixels, how many of them carry history, the MSE over them of the raw frame and of the blend, the
    blend's MSE over the frame."""
    blend, C, _ = out[-1]
    hit, _, _, ids = surface(feat)
    on = hit & (ids == SPHERE + 1)
    raw = np.asarray(S, np.float64) / spp
    return dict(pixels=int(on.sum()), carried=int((C[on, 3] > 0).sum()), weight=float(C[on, 3].mean()), raw=href.mse(raw[on], truth[on]),
                sphere=href.mse(blend[on], truth[on]), frame=href.mse(blend, truth))


# what tests/test_history_motion_sim.py prints: pixels of the sphere in the last view, of those carried (Th > 0) by the plain and by the
# motion lookup, MSE over the sphere's pixels of the raw frame, the plain blend and the motion blend, and the same two over the frame
SIM_SPHERE_PIXELS, SIM_CARRIED_PLAIN, SIM_CARRIED_MOTION = 39, 20, 38
SIM_SPHERE_RAW, SIM_SPHERE_PLAIN, SIM_SPHERE_MOTION = 0.00765731103, 0.0042707868, 0.000496352632
SIM_FRAME_PLAIN, SIM_FRAME_MOTION = 0.000911335796, 0.000882940169
