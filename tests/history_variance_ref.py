"""The variance side of the reprojected history and the filter over the blend (include/pt_amd.h: pt_history_capture_ex /
_reproject_ex with PT_HISTORY_VARIANCE, pt_history_denoise) restated in numpy float32 on top of history_ref and denoise_guided_ref:
every operation one IEEE float32 operation on arrays in the order the header states, so the results are what csrc/pt_history.h and
csrc/pt_denoise.h compute bit for bit.  Also the orbit of tests/test_history_variance_sim.py and the figures it prints."""
import numpy as np

import history_ref as href
from denoise_guided_ref import FLOOR, G, H, dist2, exp32, inv_sigma2
from history_ref import bits, dot3, f32, surface  # noqa: F401  (bits: for the tests)

DEFAULT_SIGMA = (8.0, 0.5, 1.0)  # pt_history_denoise's: sigma_color == 0 means 8


def sample_variance(noise, groups, iters):
    """vn [n, 3]: the variance of the mean of the new samples, per channel, from the fold's planes [2, n, 4]."""
    prev, q = (np.ascontiguousarray(noise, f32).reshape(2, -1, 4)[k][:, :3] for k in range(2))
    Tf = f32(iters)
    Df = f32(groups - 1) * Tf
    assert groups >= 2
    with np.errstate(all="ignore"):
        d = q - (prev * prev) / Tf
        return (np.where(d > 0, d, f32(0)) / Df).astype(f32)


def blend_variance(vn, samples, current=None, current_var=None):
    """vb [n, 3] from vn [n, 3], the current plane C [n, 4] and its variance VC [n, 4] (None: absent, all zero)."""
    n = vn.shape[0]
    C = np.zeros((n, 4), f32) if current is None else np.ascontiguousarray(current, f32).reshape(-1, 4)
    VC = np.zeros((n, 4), f32) if current_var is None else np.ascontiguousarray(current_var, f32).reshape(-1, 4)
    samples = f32(samples)
    with np.errstate(all="ignore"):
        dn = samples + C[:, 3:4]
        wn = samples / dn
        wh = C[:, 3:4] / dn
        return ((wn * wn) * vn + (wh * wh) * VC[:, :3]).astype(f32)


def capture_variance(noise, groups, iters, samples, current=None, current_var=None):
    """VK [n, 4] = {vb.xyz, +0}."""
    vb = blend_variance(sample_variance(noise, groups, iters), samples, current, current_var)
    return np.concatenate([vb, np.zeros((vb.shape[0], 1), f32)], axis=1)


def reproject_variance(cam, kept, feat, reject, kept_var, w, rows, row0=0, **opts):
    """(C, VC): history_ref.reproject with vacc beside acc — per tap that passed, vacc_k = vacc_k + b * VK(q).k after tacc; at the
    end vh = vacc / wsum; a rejected pixel gets zeros; the cap does not touch vh."""
    cap, min_dot, plane_tol, keep = href.resolve_options(**opts)
    W, Hh = int(cam.resolution[0]), int(cam.resolution[1])
    assert W == w
    pos, view, up, right = (np.array(list(v), f32) for v in (cam.position, cam.view, cam.up, cam.right))
    plx, ply = f32(cam.pixelLength[0]), f32(cam.pixelLength[1])
    hw, hh = f32(W) * f32(0.5), f32(Hh) * f32(0.5)
    K = np.ascontiguousarray(kept, f32).reshape(3, -1, 4)
    VK = np.ascontiguousarray(kept_var, f32).reshape(-1, 4)
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
        ok &= (fx >= -1) & (fx <= f32(W - 1)) & (fy >= -1) & (fy <= f32(Hh - 1))
        ax, ay = sx - fx, sy - fy
        ix = np.where(ok, fx, 0).astype(np.int64)
        iy = np.where(ok, fy, 0).astype(np.int64) - row0
        tol = plane_tol * dz
        acc, vacc = np.zeros((npix, 3), f32), np.zeros((npix, 3), f32)
        tacc, wsum = np.zeros(npix, f32), np.zeros(npix, f32)
        for j in (0, 1):
            for i in (0, 1):
                qx, qr = ix + i, iy + j
                take = ok & (qx >= 0) & (qx < w) & (qr >= 0) & (qr < rows)
                q = np.where(take, qr * w + qx, 0)
                k0, k1, k2, vk = K[0][q], K[1][q], K[2][q], VK[q]
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
                for k in range(3):
                    vacc[:, k] = np.where(take, vacc[:, k] + b * vk[:, k], vacc[:, k])
                wsum = np.where(take, wsum + b, wsum)
        ok &= wsum >= href.MIN_WEIGHT
        h = acc / wsum[:, None]
        vh = vacc / wsum[:, None]
        t = tacc / wsum
        th = np.where(t < cap, t, cap)
    C, VC = np.zeros((npix, 4), f32), np.zeros((npix, 4), f32)
    C[ok, :3], C[ok, 3] = h[ok], th[ok]
    VC[ok, :3] = vh[ok]
    return C, VC


def denoise_history(rgb_sum, planes, noise, w, rows, groups, iters, samples, current=None, current_var=None, levels=0, sigma_color=0.0,
                    sigma_normal=0.0, sigma_position=0.0, keep_albedo=False, stats=None):
    """pt_history_denoise: denoise_guided_ref.denoise_guided with another prepare — the colour is the blend of the image with C, the
    variance the blend's — and its prefilter, levels and finish as they stand there.  `stats` receives var_raw and var_0."""
    levels = levels or 5
    s0, s1, s2 = (np.asarray(planes, f32).reshape(3, rows, w, 4)[k] for k in range(3))
    inv_c, inv_n, inv_p = (inv_sigma2(s, d) for s, d in zip((sigma_color, sigma_normal, sigma_position), DEFAULT_SIGMA))
    # prepare
    hit = s1[..., 3] > 0
    den = np.where(hit, s1[..., 3], f32(1))[..., None]
    zero = np.zeros((rows, w, 3), f32)
    n = np.where(hit[..., None], s0[..., :3] / den, zero)
    a = np.where(hit[..., None], s1[..., :3] / den, zero)
    p = np.where(hit[..., None], s2[..., :3] / den, zero)
    c = href.blend(rgb_sum, samples, current).reshape(rows, w, 3)
    demod = (a > 0) & (not keep_albedo)
    safe_a = np.where(demod, a, f32(1))
    with np.errstate(all="ignore"):
        c = np.where(demod, c / safe_a, c)
        v = blend_variance(sample_variance(noise, groups, iters), samples, current, current_var).reshape(rows, w, 3)
        v = np.where(demod, v / (safe_a * safe_a), v)
        var_raw = (v[..., 0] + v[..., 1]) + v[..., 2]
    assert c.dtype == f32 and var_raw.dtype == f32
    ys, xs = np.mgrid[0:rows, 0:w]

    def tap(dy, dx):
        y, x = ys + dy, xs + dx
        inside = (y >= 0) & (y < rows) & (x >= 0) & (x < w)
        yc, xc = np.clip(y, 0, rows - 1), np.clip(x, 0, w - 1)
        return yc, xc, inside & (hit[yc, xc] == hit)

    # variance prefilter, levels, finish: the guided form's
    acc, gsum = np.zeros((rows, w), f32), np.zeros((rows, w), f32)
    with np.errstate(all="ignore"):
        for j in range(-1, 2):
            for i in range(-1, 2):
                yc, xc, take = tap(j, i)
                g = G[j + 1] * G[i + 1]
                acc = acc + np.where(take, g * var_raw[yc, xc], f32(0))
                gsum = gsum + np.where(take, g, f32(0))
        var = acc / gsum
    var_0 = var
    for l in range(levels):
        s = 1 << l
        with np.errstate(all="ignore"):
            cf = inv_c / (var + FLOOR)
            acc = np.zeros((rows, w, 3), f32)
            wsum = np.zeros((rows, w), f32)
            vsum = np.zeros((rows, w), f32)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    yc, xc, take = tap(j * s, i * s)
                    cq = c[yc, xc]
                    e = (dist2(cq, c) * cf + dist2(n[yc, xc], n) * inv_n) + dist2(p[yc, xc], p) * inv_p
                    wgt = np.where(take, (H[j + 2] * H[i + 2]) * exp32(-e), f32(0))
                    acc = acc + wgt[..., None] * cq
                    wsum = wsum + wgt
                    vsum = vsum + (wgt * wgt) * var[yc, xc]
            c = acc / wsum[..., None]
            var = vsum / (wsum * wsum)
        assert c.dtype == f32 and var.dtype == f32
    if stats is not None:
        stats.update(var_raw=var_raw.reshape(-1), var_0=var_0.reshape(-1))
    return np.where(demod, c * a, c).reshape(-1, 3)


# ---- the orbit of tests/test_history_variance_sim.py: history_ref's (cornell 96 x 54, depth 8, 8 views 3 degrees apart), the 4 spp of
# a view in 4 groups of 1 with a fold after each ------------------------------------------------------------------------------------
GROUPS = 4


def run_orbit(views, fns, spp=href.SPP, **dn_opts):
    """The command line's --denoise-history sequence over `views`, a list of (camera, S, feature planes, noise planes): from the second
    view on the history is reprojected with its variance; the view is resolved and filtered; the unfiltered blend is captured with its
    variance.  fns: capture, capture_variance, reproject_variance, blend, denoise (the host functions, or this module's).  Returns per
    view (blend, filtered blend, C, VC, K, VK)."""
    out = []
    K = VK = kept_cam = None
    for cam, S, feat, noise in views:
        C, VC = (None, None) if K is None else fns["reproject_variance"](kept_cam, K, feat, VK)
        blend = fns["blend"](S, spp, C)
        filtered = fns["denoise"](S, feat, noise, spp, C, VC, **dn_opts)
        K, VK, kept_cam = fns["capture"](S, feat, spp, C), fns["capture_variance"](noise, spp, C, VC), cam
        out.append((blend, filtered, C, VC, K, VK))
    return out


def host_functions(reject, w, h, groups=GROUPS, iters=href.SPP):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    return dict(capture=lambda S, feat, spp, C: capi.history_capture_host(S, feat, spp, C),
                capture_variance=lambda noise, spp, C, VC: capi.history_capture_variance_host(noise, groups, iters, spp, C, VC),
                reproject_variance=lambda cam, K, feat, VK: capi.history_reproject_variance_host(cam, K, feat, reject, VK, w, h),
                blend=lambda S, spp, C: capi.history_blend_host(S, spp, C),
                denoise=lambda S, feat, noise, spp, C, VC, **o: capi.history_denoise_host(S, feat, noise, w, h, groups, iters, spp, C, VC, **o))


def ref_functions(reject, w, h, groups=GROUPS, iters=href.SPP):
    return dict(capture=href.capture, capture_variance=lambda noise, spp, C, VC: capture_variance(noise, groups, iters, spp, C, VC),
                reproject_variance=lambda cam, K, feat, VK: reproject_variance(cam, K, feat, reject, VK, w, h),
                blend=href.blend,
                denoise=lambda S, feat, noise, spp, C, VC, **o: denoise_history(S, feat, noise, w, h, groups, iters, spp, C, VC, **o))


def calibration(VK, blend, truth):
    """sum over pixels and channels of the carried variance VK against the actual squared error of the blend: (sum var, sum err^2)."""
    err = np.asarray(blend, np.float64) - truth
    return float(np.asarray(VK, np.float64)[:, :3].sum()), float((err ** 2).sum())


# what tests/test_history_variance_sim.py prints (MSE against the 1024-spp frame at the last camera), and the exact build reproduces on
# the device: the filtered blend, pt_denoise_guided on the last view's own 4 spp, the ratios of the first against history_ref.SIM_CARRIED
# and against the second, and the calibration of the last view — the sum of the captured variance VK against the squared error of the
# blend it belongs to, over pixels and channels (2.19: the carried variance reads high, as the header says it must)
SIM_FILTERED, SIM_GUIDED_ALONE = 0.000139623228, 0.000453949415
SIM_FILTERED_OF_CARRIED, SIM_FILTERED_OF_GUIDED = 0.3086, 0.3076
SIM_SUM_VAR, SIM_SUM_ERR2 = 15.3941732194, 7.03736819742
