"""The reprojected sample history of include/pt_amd.h (pt_history_capture / _reproject / _resolve) restated in numpy float32: every
operation below is one IEEE float32 operation on arrays, in the order the header states, so the result is what csrc/pt_history.h
computes bit for bit.  Also the adversarial inputs the host and the GPU tests share."""
import numpy as np

f32 = np.float32
CAP, MIN_DOT, PLANE_TOL = f32(32.0), f32(0.9), f32(0.02)
MIN_WEIGHT = f32(0.015625)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def surface(feat):
    """hit [n], n [n, 3], p [n, 3], id [n] int32 from the feature SUM planes [3, n, 4] (pt_denoise's prepare)."""
    feat = np.ascontiguousarray(feat, f32).reshape(3, -1, 4)
    s0, s1, s2 = feat
    hit = s1[:, 3] > 0
    with np.errstate(all="ignore"):
        n = np.where(hit[:, None], s0[:, :3] / s1[:, 3:4], f32(0)).astype(f32)
        p = np.where(hit[:, None], s2[:, :3] / s1[:, 3:4], f32(0)).astype(f32)
    ids = np.where(hit, np.ascontiguousarray(s2[:, 3]).view(np.int32), 0).astype(np.int32)
    return hit, n, p, ids


def blend(rgb_sum, samples, current=None):
    S = np.ascontiguousarray(rgb_sum, f32).reshape(-1, 3)
    C = np.zeros((S.shape[0], 4), f32) if current is None else np.ascontiguousarray(current, f32).reshape(-1, 4)
    samples = f32(samples)
    with np.errstate(all="ignore"):
        m = C[:, :3] * C[:, 3:4]
        a = S + m
        d = samples + C[:, 3:4]
        return (a / d).astype(f32)


def capture(rgb_sum, feat, samples, current=None):
    S = np.ascontiguousarray(rgb_sum, f32).reshape(-1, 3)
    n_pix = S.shape[0]
    C = np.zeros((n_pix, 4), f32) if current is None else np.ascontiguousarray(current, f32).reshape(-1, 4)
    hit, n, p, ids = surface(feat)
    K = np.zeros((3, n_pix, 4), f32)
    K[0, :, :3] = blend(S, samples, C)
    with np.errstate(all="ignore"):
        K[0, :, 3] = f32(samples) + C[:, 3]
    K[1, :, :3] = p
    K[1, :, 3] = ids.view(f32)
    K[2, :, :3] = n
    return K


def resolve_options(cap=0.0, min_normal_dot=0.0, plane_tol=0.0, keep_view_dependent=False):
    cap, md, pt = f32(cap), f32(min_normal_dot), f32(plane_tol)
    return (CAP if cap == 0 else cap, MIN_DOT if md == 0 else md, PLANE_TOL if pt == 0 else pt, bool(keep_view_dependent))


def reproject(cam, kept, feat, reject, w, rows, row0=0, stats=None, **opts):
    """cam: anything with resolution, position, view, up, right, pixelLength (a capi.PtCamera).  stats: a dict that receives sx, sy, dz
    and wsum per pixel (whatever the pixel's fate), for tests that plant conditions."""
    cap, min_dot, plane_tol, keep = resolve_options(**opts)
    W, H = int(cam.resolution[0]), int(cam.resolution[1])
    assert W == w
    pos, view, up, right = (np.array(list(v), f32) for v in (cam.position, cam.view, cam.up, cam.right))
    plx, ply = f32(cam.pixelLength[0]), f32(cam.pixelLength[1])
    hw, hh = f32(W) * f32(0.5), f32(H) * f32(0.5)
    K = np.ascontiguousarray(kept, f32).reshape(3, -1, 4)
    npix = w * rows
    hit, n, p, ids = surface(feat)
    reject = np.ascontiguousarray(reject, np.uint8).reshape(-1)
    ok = hit.copy()
    if not keep:
        inside = (ids >= 1) & (ids <= reject.size)
        listed = np.zeros(npix, bool)
        listed[inside] = reject[ids[inside] - 1] != 0
        ok &= inside & ~listed
    with np.errstate(all="ignore"):
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
        acc = np.zeros((npix, 3), f32)
        tacc = np.zeros(npix, f32)
        wsum = np.zeros(npix, f32)
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
                wsum = np.where(take, wsum + b, wsum)
        ok &= wsum >= MIN_WEIGHT
        h = acc / wsum[:, None]
        t = tacc / wsum
        th = np.where(t < cap, t, cap)
    if stats is not None:
        stats.update(sx=sx, sy=sy, dz=dz, wsum=wsum, hit=hit)
    C = np.zeros((npix, 4), f32)
    C[ok, :3] = h[ok]
    C[ok, 3] = th[ok]
    return C


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
class Cam:
    """A camera with the fields the lookup reads; to_capi() gives the PtCamera the library takes."""

    def __init__(self, w, h, position=(0.25, 0.5, -6.0), view=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), right=(-1.0, 0.0, 0.0), pixel_length=(0.03125, 0.03125)):
        self.resolution = (w, h)
        self.position, self.view, self.up, self.right, self.pixelLength = position, view, up, right, pixel_length

    def to_capi(self):
        from cosc_4397_pathtracing_raytracing_project_amd import capi
        c = capi.PtCamera()
        c.resolution[:] = self.resolution
        c.position[:], c.view[:], c.up[:], c.right[:] = self.position, self.view, self.up, self.right
        c.lookAt[:] = (0.0, 0.0, 0.0)
        c.fov[:] = (45.0, 45.0)
        c.pixelLength[:] = self.pixelLength
        return c


SHAPES = [(1, 1), (2, 2), (5, 3), (97, 61)]
ROW0 = [0, 7]
NUM_GEOMS = 6


def point_at(cam, sx, sy, depth):
    """A world point that the camera's axis-aligned frame (view +z, up +y, right -x, pixel lengths powers of two) projects to EXACTLY
    (sx, sy) when sx, sy and depth are short binary fractions: every operation of the lookup is then exact."""
    plx, ply = cam.pixelLength
    hw, hh = cam.resolution[0] * 0.5, cam.resolution[1] * 0.5
    vr = (hw - sx) * depth * plx   # v . right
    vu = (hh - sy) * depth * ply   # v . up
    return (cam.position[0] - vr, cam.position[1] + vu, cam.position[2] + depth)


def adversarial(w, rows, row0, seed=0):
    """(cam, kept [3, n, 4], feat [3, n, 4], reject [NUM_GEOMS]) for a tile of w x rows at frame row row0 of a frame w x (row0 + rows + 3):
    random surfaces and ids, then planted pixels — NaN / infinite positions, dz <= 0, sx / sy exactly on integers, at -1, at W - 1 and
    beyond both, taps with Tk == 0, and pairs of taps whose bilinear weights sum to just under and exactly 1/64."""
    rng = np.random.default_rng(1000 * seed + 100 * w + 10 * rows + row0)
    H = row0 + rows + 3
    cam = Cam(w, H)
    n = w * rows
    normal = np.array([0.0, 0.0, -1.0], f32)
    # the kept view: a wall at depth 8 (z = 2) seen by the kept camera, every pixel its own point; random colours, weights, ids
    kept = np.zeros((3, n, 4), f32)
    kept[0, :, :3] = rng.random((n, 3), dtype=f32)
    kept[0, :, 3] = rng.choice(np.array([0.0, 1.0, 4.0, 31.5, 40.0], f32), n)           # Tk == 0 among them
    xs, ys = np.meshgrid(np.arange(w), np.arange(row0, row0 + rows))
    for i, (x, y) in enumerate(zip(xs.ravel(), ys.ravel())):
        kept[1, i, :3] = point_at(cam, x + 0.5, y + 0.5, 8.0)
    kept[1, :, 3] = rng.integers(1, NUM_GEOMS + 1, n).astype(np.int32).view(f32)
    kept[2, :, :3] = normal
    tilt = rng.random(n) < 0.2
    kept[2, tilt, :3] = np.array([0.6, 0.0, -0.8], f32)                                   # fails the default normal test, passes 0.5
    # the current view's feature sums over 4 iterations: points on the same wall at random screen positions of the kept camera
    hits = f32(4.0)
    feat = np.zeros((3, n, 4), f32)
    sx = (rng.integers(-3 * 4, (w + 2) * 4, n) / 4.0).astype(f32)                        # quarter pixels: integers among them
    sy = (rng.integers((row0 - 3) * 4, (H + 2) * 4, n) / 4.0).astype(f32)
    depth = rng.choice(np.array([8.0, 8.0, 8.0, 8.125, 9.0], f32), n)                    # on the plane, within the tolerance, off it
    plant = {}
    if n >= 15:
        order = rng.permutation(n)
        names = ["nan", "inf", "behind", "dz0", "left_edge", "right_edge", "top_edge", "bottom_edge", "past_left", "past_right", "past_top", "past_bottom",
                 "under_64th", "at_64th", "miss"]
        plant = {name: int(order[k]) for k, name in enumerate(names)}
        sx[plant["left_edge"]], sx[plant["right_edge"]] = -1.0, w - 1.0
        sy[plant["top_edge"]], sy[plant["bottom_edge"]] = -1.0, H - 1.0
        sx[plant["past_left"]], sx[plant["past_right"]] = -1.25, float(w)
        sy[plant["past_top"]], sy[plant["past_bottom"]] = -1.5, float(H)
        # ax = 1/64 with only the right column inside (sx in [-1, 0)): wsum = 1/64 exactly when ay's two rows both pass; one ulp less under it
        sx[plant["at_64th"]] = -1.0 + 0.015625
        sx[plant["under_64th"]] = -1.0 + 0.015625 - 2.0 ** -16
        for name in ("at_64th", "under_64th"):
            sy[plant[name]] = row0 + 0.5
            depth[plant[name]] = 8.0
        for name in ("left_edge", "right_edge", "past_left", "past_right"):
            sy[plant[name]] = row0 + 0.25
        for name in ("top_edge", "bottom_edge", "past_top", "past_bottom"):
            sx[plant[name]] = 0.25
    for i in range(n):
        feat[2, i, :3] = np.array(point_at(cam, float(sx[i]), float(sy[i]), float(depth[i])), f32) * hits
    feat[0, :, :3] = normal * hits
    feat[1, :, :3] = 0.5 * hits
    feat[1, :, 3] = hits
    feat[2, :, 3] = rng.integers(1, NUM_GEOMS + 1, n).astype(np.int32).view(f32)
    # most pixels look at the id the kept pixel under them has, so that taps pass
    same = rng.random(n) < 0.7
    ix = np.clip(np.floor(sx).astype(int), 0, w - 1)
    iy = np.clip(np.floor(sy).astype(int) - row0, 0, rows - 1)
    feat[2, same, 3] = kept[1, (iy * w + ix)[same], 3]
    if plant:
        for name in ("at_64th", "under_64th"):                                            # the column x = 0 passes every test for these two
            i = plant[name]
            col = np.arange(rows) * w
            feat[2, i, 3] = np.array([1], np.int32).view(f32)[0]
            kept[1, col, 3] = feat[2, i, 3]
            kept[0, col, 3] = 4.0
            kept[2, col, :3] = normal
        feat[2, plant["nan"], 0] = np.nan
        feat[2, plant["inf"], 1] = np.inf
        feat[2, plant["behind"], :3] = np.array(point_at(cam, 1.0, row0 + 1.0, -4.0), f32) * hits
        feat[2, plant["dz0"], :3] = np.array((1.0, 1.0, cam.position[2]), f32) * hits
        feat[:, plant["miss"], :] = 0
    reject = np.zeros(NUM_GEOMS, np.uint8)
    reject[2] = 1
    return cam, kept, feat, reject, plant


OPTION_SETS = {
    "defaults": dict(),
    "tests_off": dict(min_normal_dot=-1.0, plane_tol=-1.0),
    "custom": dict(cap=8.0, min_normal_dot=0.5, plane_tol=0.25),
    "keep_view_dependent": dict(keep_view_dependent=True),
}


# ---- the orbit of tests/test_history_sim.py: cornell 96 x 54, depth 8, 8 views 3 degrees apart around LOOKAT, 4 spp per view -----------
RES, FRAMES, SPP, STEP_DEG = (96, 54), 8, 4, 3.0
TRUTH_FIRST, TRUTH_SPP, UNIFORM_SPP = 100001, 1024, 32


def orbit_eye(frame, step_deg=STEP_DEG, radius=10.5, lookat=(0.0, 5.0, 0.0)):
    a = np.deg2rad(step_deg * frame)
    return (lookat[0] + radius * float(np.sin(a)), lookat[1], lookat[2] + radius * float(np.cos(a)))


def orbit_scene_paths(directory, text_fn=None, frames=FRAMES):
    """Scene files of the orbit's views: the same scene, EYE moved (text_fn: camera_scenes' cornell_text / random_text)."""
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    import camera_scenes
    text_fn = text_fn or camera_scenes.cornell_text
    return [scenes.write_scene(text_fn(eye=orbit_eye(f)), str(directory / f"{text_fn.__name__}_orbit{f}.txt")) for f in range(frames)]


def pack_features(v):
    """features_ref's per-name arrays -> the planes [3, n, 4] pt_readback_features gives."""
    n = v["hits"].shape[0]
    planes = np.zeros((3, n, 4), f32)
    planes[0, :, :3], planes[0, :, 3] = v["normal"], v["depth"]
    planes[1, :, :3], planes[1, :, 3] = v["albedo"], v["hits"]
    planes[2, :, :3], planes[2, :, 3] = v["position"], np.ascontiguousarray(v["object_id"], np.int32).view(f32)
    return planes


def run_orbit(views, capture_fn, reproject_fn, blend_fn, spp=SPP):
    """The command line's sequence over `views`, a list of (camera, S, feature planes): from the second view on the history is
    reprojected, then the view is resolved, then captured.  Returns the resolved images and the current planes."""
    out, currents = [], []
    kept = kept_cam = None
    for cam, S, feat in views:
        C = None if kept is None else reproject_fn(kept_cam, kept, feat)
        out.append(blend_fn(S, spp, C))
        currents.append(C)
        kept, kept_cam = capture_fn(S, feat, spp, C), cam
    return out, currents


def mse(img, truth):
    return float(((np.asarray(img, np.float64) - truth) ** 2).mean())


# what tests/test_history_sim.py prints (MSE against the 1024-spp frame at the last camera), and the exact build reproduces on the device
SIM_RAW, SIM_UNIFORM, SIM_CARRIED, SIM_CARRIED_CAP8, SIM_STILL = 0.00657237, 0.000830143, 0.000452506, 0.00111436, 0.000944142
