"""Moments with the history (include/pt_amd.h: pt_history_capture_ex / _reproject_ex with PT_HISTORY_MOMENTS, pt_history_denoise_ex)
restated in numpy float32 on top of history_ref and history_variance_ref: every operation one IEEE float32 operation on arrays in the
order the header states, so the results are what csrc/pt_history.h and csrc/pt_denoise.h compute bit for bit.  Also the orbits of
tests/test_history_moments_sim.py and the figures it prints."""
import numpy as np

import history_ref as href
import history_variance_ref as vref
from denoise_guided_ref import FLOOR, G, H, dist2, exp32, inv_sigma2
from history_ref import bits, f32  # noqa: F401  (bits: for the tests)

R_MAX = f32(0.3)     # PT_HISTORY_MOMENTS_R_MAX
MARK = f32(-1.0)     # var_raw of a pixel marked for the spatial estimate
RADIUS = 3           # of the spatial estimate's window
DEFAULT_SIGMA = vref.DEFAULT_SIGMA  # pt_history_denoise_ex's: sigma_color == 0 means 8


def _planes(n, current, current_var):
    C = np.zeros((n, 4), f32) if current is None else np.ascontiguousarray(current, f32).reshape(-1, 4)
    VC = np.zeros((n, 4), f32) if current_var is None else np.ascontiguousarray(current_var, f32).reshape(-1, 4)
    return C, VC


def blend_moments(rgb_sum, samples, current=None, current_var=None):
    """{m2b.xyz, rb} [n, 4] from the SUM image [n, 3], the current plane C and its moments VC = {m2h.xyz, rh} (None: absent, all zero)."""
    S = np.ascontiguousarray(rgb_sum, f32).reshape(-1, 3)
    C, VC = _planes(S.shape[0], current, current_var)
    samples = f32(samples)
    with np.errstate(all="ignore"):
        x = S / samples
        dn = samples + C[:, 3:4]
        wn = samples / dn
        wh = C[:, 3:4] / dn
        m2b = wn * (x * x) + wh * VC[:, :3]
        rb = wn * wn + (wh * wh) * VC[:, 3:4]
    out = np.concatenate([m2b, rb], axis=1)
    assert out.dtype == f32
    return out


capture_moments = blend_moments  # VK = {m2b.xyz, rb}


def reproject_moments(cam, kept, feat, reject, kept_var, w, rows, row0=0, **opts):
    """(C, VC): history_variance_ref.reproject_variance over four components.  Its three are the same operations on x, y, z; the fourth
    is run through it once more in x's place: vacc_w = vacc_w + b * VK(q).w after tacc, VC.w = vacc_w / wsum, 0 where rejected."""
    VK = np.ascontiguousarray(kept_var, f32).reshape(-1, 4)
    C, VC = vref.reproject_variance(cam, kept, feat, reject, VK, w, rows, row0, **opts)
    w_first = np.zeros_like(VK)
    w_first[:, 0] = VK[:, 3]
    VC[:, 3] = vref.reproject_variance(cam, kept, feat, reject, w_first, w, rows, row0, **opts)[1][:, 0]
    return C, VC


def denoise_moments(rgb_sum, planes, w, rows, samples, current=None, current_var=None, levels=0, sigma_color=0.0, sigma_normal=0.0,
                    sigma_position=0.0, keep_albedo=False, spatial=True, stats=None):
    """pt_history_denoise_ex with PT_HISTORY_MOMENTS.  spatial=False: the marked pixels get var_raw = 0 instead of the spatial estimate
    (the comparison of tests/test_history_moments_sim.py; the library has no such switch).  `stats` receives mark, var_raw (after the
    spatial step) and var_0."""
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
    cb = href.blend(rgb_sum, samples, current).reshape(rows, w, 3)
    mom = blend_moments(rgb_sum, samples, current, current_var).reshape(rows, w, 4)
    m2b, rb = mom[..., :3], mom[..., 3]
    demod = (a > 0) & (not keep_albedo)
    safe_a = np.where(demod, a, f32(1))
    with np.errstate(all="ignore"):
        c = np.where(demod, cb / safe_a, cb)
        d = m2b - cb * cb
        d = np.where(d > 0, d, f32(0))
        f = rb / (f32(1) - rb)
        v = d * f[..., None]
        v = np.where(demod, v / (safe_a * safe_a), v)
        mark = ~(rb <= R_MAX)
        var_raw = np.where(mark, MARK, (v[..., 0] + v[..., 1]) + v[..., 2]).astype(f32)
    assert c.dtype == f32 and var_raw.dtype == f32
    ys, xs = np.mgrid[0:rows, 0:w]

    def tap(dy, dx):
        y, x = ys + dy, xs + dx
        inside = (y >= 0) & (y < rows) & (x >= 0) & (x < w)
        yc, xc = np.clip(y, 0, rows - 1), np.clip(x, 0, w - 1)
        return yc, xc, inside & (hit[yc, xc] == hit)

    # the spatial estimate, for the marked pixels (computed for all, taken by those)
    if spatial:
        wsum = np.zeros((rows, w), f32)
        s1s, s2s = np.zeros((rows, w, 3), f32), np.zeros((rows, w, 3), f32)
        with np.errstate(all="ignore"):
            for j in range(-RADIUS, RADIUS + 1):
                for i in range(-RADIUS, RADIUS + 1):
                    yc, xc, take = tap(j, i)
                    cq = c[yc, xc]
                    e = dist2(n[yc, xc], n) * inv_n + dist2(p[yc, xc], p) * inv_p
                    wgt = exp32(-e)
                    wsum = np.where(take, wsum + wgt, wsum)
                    s1s = np.where(take[..., None], s1s + wgt[..., None] * cq, s1s)
                    s2s = np.where(take[..., None], s2s + wgt[..., None] * (cq * cq), s2s)
            mean, u = s1s / wsum[..., None], s2s / wsum[..., None]
            ds = u - mean * mean
            ds = np.where(ds > 0, ds, f32(0))
            var_raw = np.where(mark, (ds[..., 0] + ds[..., 1]) + ds[..., 2], var_raw).astype(f32)
    else:
        var_raw = np.where(mark, f32(0), var_raw)
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
        stats.update(mark=mark.reshape(-1), var_raw=var_raw.reshape(-1), var_0=var_0.reshape(-1), hit=hit.reshape(-1))
    return np.where(demod, c * a, c).reshape(-1, 3)


# ---- inputs the host and the GPU tests share ---------------------------------------------------------------------------------------
MARK_PATTERNS = ("none", "all", "one_lane", "checkerboard")


def current_planes(w, rows, pattern, seed=0):
    """C, VC [n, 4] of a lookup with moments whose marks follow `pattern`: rh = 1/8 (unmarked: the temporal branch) or 1/2 (marked) with
    Th = 7 against samples = 1, so that rb = (1/8)^2 + (7/8)^2 rh is 0.111 or 0.398.  one_lane: pixel 5 of row 1 if the frame has it,
    the last pixel otherwise.  m2h is the colour's square plus a spread many decades wide, zeros among it."""
    n = w * rows
    rng = np.random.default_rng(977 * seed + 31 * w + rows)
    C, VC = np.zeros((n, 4), f32), np.zeros((n, 4), f32)
    C[:, :3] = rng.random((n, 3), dtype=f32)
    C[:, 3] = 7.0
    spread = (rng.random((n, 3), dtype=f32) * f32(10.0) ** rng.integers(-8, 0, (n, 3)).astype(f32)).astype(f32)
    spread[rng.random(n) < 0.15] = 0
    VC[:, :3] = C[:, :3] * C[:, :3] + spread
    ys, xs = np.divmod(np.arange(n), w)
    marked = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "checkerboard": (xs + ys) % 2 == 1,
              "one_lane": np.arange(n) == (w + 5 if w > 5 and rows > 1 else n - 1)}[pattern]
    VC[:, 3] = np.where(marked, f32(0.5), f32(0.125))
    return C, VC, marked


# ---- the orbits of tests/test_history_moments_sim.py: history_ref's (cornell 96 x 54, depth 8, 8 views 3 degrees apart) at 1 spp per
# view, view f rendering iteration f + 1; and the same at history_ref's 4 spp per view, without a fold -------------------------------
def run_orbit(views, fns, spp, **dn_opts):
    """The command line's --denoise-history --history-moments sequence over `views`, a list of (camera, S, feature planes): from the
    second view on the history is reprojected with its moments; the view is resolved and filtered; the unfiltered blend is captured
    with its moments.  fns: capture, capture_moments, reproject_moments, blend, denoise (the host functions, or this module's).
    Returns per view (blend, filtered blend, C, VC, K, VK)."""
    out = []
    K = VK = kept_cam = None
    for cam, S, feat in views:
        C, VC = (None, None) if K is None else fns["reproject_moments"](kept_cam, K, feat, VK)
        blend = fns["blend"](S, spp, C)
        filtered = fns["denoise"](S, feat, spp, C, VC, **dn_opts)
        K, VK, kept_cam = fns["capture"](S, feat, spp, C), fns["capture_moments"](S, spp, C, VC), cam
        out.append((blend, filtered, C, VC, K, VK))
    return out


def host_functions(reject, w, h):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    return dict(capture=lambda S, feat, spp, C: capi.history_capture_host(S, feat, spp, C),
                capture_moments=lambda S, spp, C, VC: capi.history_capture_moments_host(S, spp, C, VC),
                reproject_moments=lambda cam, K, feat, VK: capi.history_reproject_moments_host(cam, K, feat, reject, VK, w, h),
                blend=lambda S, spp, C: capi.history_blend_host(S, spp, C),
                denoise=lambda S, feat, spp, C, VC, **o: capi.history_denoise_moments_host(S, feat, w, h, spp, C, VC, **o))


def ref_functions(reject, w, h):
    return dict(capture=href.capture, capture_moments=capture_moments,
                reproject_moments=lambda cam, K, feat, VK: reproject_moments(cam, K, feat, reject, VK, w, h),
                blend=href.blend, denoise=lambda S, feat, spp, C, VC, **o: denoise_moments(S, feat, w, h, spp, C, VC, **o))


def marked_share(mark, hit, blend, truth):
    """(the share of marked hit pixels in the frame, their share of the blend's squared error)."""
    fresh = np.asarray(mark, bool) & np.asarray(hit, bool)
    err2 = ((np.asarray(blend, np.float64) - truth) ** 2).sum(axis=1)
    return float(fresh.mean()), float(err2[fresh].sum() / err2.sum())


# what tests/test_history_moments_sim.py prints (MSE against the 1024-spp frame at the last camera), and the exact build reproduces on
# the device.  1 spp per view: the blend, the filtered blend, pt_denoise_host on the last view's own 1 spp, the filtered blend without
# the spatial estimate (marked pixels get variance 0), the share of marked hit pixels and their share of the blend's squared error.
# 4 spp per view: the filtered blend (against history_ref.SIM_CARRIED and history_variance_ref.SIM_FILTERED).
SIM_BLEND, SIM_FILTERED, SIM_PLAIN_ALONE, SIM_NO_SPATIAL = 0.00157661377, 0.000407981136, 0.00247956009, 0.000586685609
SIM_MARKED_SHARE, SIM_MARKED_ERR_SHARE = 0.00887345679, 0.285338754
SIM_FILTERED_4SPP = 0.000139798314
