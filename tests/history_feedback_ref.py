"""The feedback of include/pt_amd.h (pt_history_reproject_ex / _capture_ex with PT_HISTORY_FEEDBACK, pt_history_denoise_feedback)
restated in numpy float32 on top of history_moments_ref and history_motion_ref: every operation one IEEE float32 operation on arrays
in the order the header states, so the results are what csrc/pt_history.h and csrc/pt_denoise.h compute bit for bit.  Also the inputs
the host and the GPU tests share, and the orbits of tests/test_history_feedback_sim.py with the figures it prints."""
import numpy as np

import history_moments_ref as mref
import history_motion_ref as moref
import history_ref as href
from denoise_guided_ref import FLOOR, G, H, dist2, exp32, inv_sigma2
from history_ref import bits, f32  # noqa: F401  (bits: for the tests)

FEEDBACK = 16  # PT_HISTORY_FEEDBACK


def reproject_feedback(cam, kept, feat, reject, kept_var, kept_fb, w, rows, row0=0, table=None, kind=None, **opts):
    """(C, VC, FC).  C and VC are the moments lookup's (with the motion table: the motion lookup's of the moments kind).  FC's four
    components are interpolated exactly as VC's four are — facc_k = facc_k + b * FK(q).k after vacc, FC.k = facc_k / wsum, 0 where the
    pixel is rejected — so the same lookup is run once more with FK in VK's place."""
    FK = np.ascontiguousarray(kept_fb, f32).reshape(-1, 4)
    if table is None:
        C, VC = mref.reproject_moments(cam, kept, feat, reject, kept_var, w, rows, row0, **opts)
        FC = mref.reproject_moments(cam, kept, feat, reject, FK, w, rows, row0, **opts)[1]
    else:
        flags = moref.MOTION | moref.MOMENTS
        C, VC = moref.reproject_motion(cam, kept, feat, reject, table, kind, w, rows, row0, flags=flags, kept_var=kept_var, **opts)
        FC = moref.reproject_motion(cam, kept, feat, reject, table, kind, w, rows, row0, flags=flags, kept_var=FK, **opts)[1]
    return C, VC, FC


def denoise_feedback(rgb_sum, planes, w, rows, samples, extra=None, current=None, current_var=None, current_fb=None, level=0, variance=None,
                     levels=0, sigma_color=0.0, sigma_normal=0.0, sigma_position=0.0, keep_albedo=False, stats=None):
    """pt_history_denoise_feedback: (the filtered image [n, 3], the tap plane P [n, 4]).  `stats` receives mark, var_raw (after the
    spatial step) and var_0."""
    levels = levels or 5
    level = level or 1
    variance = 1 if variance is None else variance  # the rule; the defaults: level 1, rule 1
    assert 1 <= level <= levels and variance in (0, 1)
    n_pix = w * rows
    ns = f32(samples) if extra is None else f32(samples) + np.ascontiguousarray(extra, f32).reshape(-1, 1)  # one add, before anything else
    s0, s1, s2 = (np.asarray(planes, f32).reshape(3, rows, w, 4)[k] for k in range(3))
    inv_c, inv_n, inv_p = (inv_sigma2(s, d) for s, d in zip((sigma_color, sigma_normal, sigma_position), mref.DEFAULT_SIGMA))
    # prepare: everything the moments prepare computes, the same way
    hit = s1[..., 3] > 0
    den = np.where(hit, s1[..., 3], f32(1))[..., None]
    zero = np.zeros((rows, w, 3), f32)
    n = np.where(hit[..., None], s0[..., :3] / den, zero)
    a = np.where(hit[..., None], s1[..., :3] / den, zero)
    p = np.where(hit[..., None], s2[..., :3] / den, zero)
    cb = href.blend(rgb_sum, ns, current).reshape(rows, w, 3)
    mom = mref.blend_moments(rgb_sum, ns, current, current_var).reshape(rows, w, 4)
    m2b, rb = mom[..., :3], mom[..., 3]
    # the colour that is filtered: the new samples with the FILTERED history, weighted as the raw blend (its .w is C's)
    Cw = np.zeros((n_pix, 1), f32) if current is None else np.ascontiguousarray(current, f32).reshape(-1, 4)[:, 3:4]
    FC = np.zeros((n_pix, 4), f32) if current_fb is None else np.ascontiguousarray(current_fb, f32).reshape(-1, 4)
    cf = href.blend(rgb_sum, ns, np.concatenate([FC[:, :3], Cw], axis=1)).reshape(rows, w, 3)
    demod = (a > 0) & (not keep_albedo)
    safe_a = np.where(demod, a, f32(1))
    with np.errstate(all="ignore"):
        c = np.where(demod, cf / safe_a, cf)
        d = m2b - cb * cb
        d = np.where(d > 0, d, f32(0))
        mark = ~(rb <= mref.R_MAX)
        if variance == 0:  # the moments form's, from the raw chain
            f = rb / (f32(1) - rb)
            v = d * f[..., None]
            v = np.where(demod, v / (safe_a * safe_a), v)
            var_t = (v[..., 0] + v[..., 1]) + v[..., 2]
        else:  # the new view's variance and the one the filtered history carries
            g = f32(1) - rb
            s = d / g[..., None]
            s = np.where(demod, s / (safe_a * safe_a), s)
            sv = (s[..., 0] + s[..., 1]) + s[..., 2]
            dn = ns + Cw
            wn = (ns / dn).reshape(rows, w)
            wh = (Cw / dn).reshape(rows, w)
            var_t = (wn * wn) * sv + (wh * wh) * FC[:, 3].reshape(rows, w)
        var_raw = np.where(mark, mref.MARK, var_t).astype(f32)
    assert c.dtype == f32 and var_raw.dtype == f32
    ys, xs = np.mgrid[0:rows, 0:w]

    def tap(dy, dx):
        y, x = ys + dy, xs + dx
        inside = (y >= 0) & (y < rows) & (x >= 0) & (x < w)
        yc, xc = np.clip(y, 0, rows - 1), np.clip(x, 0, w - 1)
        return yc, xc, inside & (hit[yc, xc] == hit)

    # the moments form's spatial estimate, over the colour that is filtered
    wsum = np.zeros((rows, w), f32)
    s1s, s2s = np.zeros((rows, w, 3), f32), np.zeros((rows, w, 3), f32)
    with np.errstate(all="ignore"):
        for j in range(-mref.RADIUS, mref.RADIUS + 1):
            for i in range(-mref.RADIUS, mref.RADIUS + 1):
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
    # variance prefilter and levels: the guided form's; the tap after level `level` - 1
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
    P = None
    for l in range(levels):
        s = 1 << l
        with np.errstate(all="ignore"):
            cfac = inv_c / (var + FLOOR)
            acc = np.zeros((rows, w, 3), f32)
            wsum = np.zeros((rows, w), f32)
            vsum = np.zeros((rows, w), f32)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    yc, xc, take = tap(j * s, i * s)
                    cq = c[yc, xc]
                    e = (dist2(cq, c) * cfac + dist2(n[yc, xc], n) * inv_n) + dist2(p[yc, xc], p) * inv_p
                    wgt = np.where(take, (H[j + 2] * H[i + 2]) * exp32(-e), f32(0))
                    acc = acc + wgt[..., None] * cq
                    wsum = wsum + wgt
                    vsum = vsum + (wgt * wgt) * var[yc, xc]
            c = acc / wsum[..., None]
            var = vsum / (wsum * wsum)
        assert c.dtype == f32 and var.dtype == f32
        if l + 1 == level:
            P = np.concatenate([np.where(demod, c * a, c).reshape(-1, 3), var.reshape(-1, 1)], axis=1)
    if stats is not None:
        stats.update(mark=mark.reshape(-1), var_raw=var_raw.reshape(-1), var_0=var_0.reshape(-1), hit=hit.reshape(-1))
    return np.where(demod, c * a, c).reshape(-1, 3), P


# ---- inputs the host and the GPU tests share ---------------------------------------------------------------------------------------
# (w, rows, row0, frame rows): a tile whose width is no multiple of anything and whose row groups are partial at every level, in the
# middle of a taller frame; one wave's width, four rows; one short row
SHAPES = [(37, 23, 5, 33), (64, 4, 0, 7), (5, 1, 0, 4)]
SHAPE_IDS = ["37x23", "64x4", "5x1"]


def kept_feedback(n, seed):
    """FK [n, 4]: a colour, and a variance many decades wide with zeros among it."""
    rng = np.random.default_rng(seed)
    fk = np.zeros((n, 4), f32)
    fk[:, :3] = rng.random((n, 3), dtype=f32)
    fk[:, 3] = (rng.random(n, dtype=f32) * f32(10.0) ** rng.integers(-10, 0, n).astype(f32)).astype(f32)
    fk[rng.random(n) < 0.15, 3] = 0
    return fk


def kept_moments(n, seed):
    """VK [n, 4] as tests/test_history_moments_host.py draws it: second moments many decades apart, zeros among them; r in 1/32 .. 1."""
    rng = np.random.default_rng(seed)
    vk = np.zeros((n, 4), f32)
    vk[:, :3] = (rng.random((n, 3), dtype=f32) * f32(10.0) ** rng.integers(-12, 1, (n, 3)).astype(f32)).astype(f32)
    vk[rng.random(n) < 0.15, :3] = 0
    vk[:, 3] = rng.choice(np.array([1.0, 0.5, 0.3, 0.25, 0.125, 0.03125], f32), n)
    return vk


def lookup_arrays(w, rows, row0, frame_rows):
    """(cam, kept, feat, reject, table, kind, VK, FK) for a tile of w x rows at frame row row0: history_motion_ref's adversarial arrays
    (moved pixels that carry, kinds that carry nothing) under a kept camera whose frame has frame_rows rows."""
    _, kept, feat, reject, _, table, kind, _ = moref.adversarial(w, rows, row0)
    n = w * rows
    return href.Cam(w, frame_rows), kept, feat, reject, table, kind, kept_moments(n, 7 * n + 1), kept_feedback(n, 7 * n + 2)


def current_planes(n, seed, cap=32.0):
    """C, VC, FC [n, 4] of a lookup that carried most pixels: weights up to the cap (reached by a fifth), a tenth with one sample behind
    them, rejected pixels all zero; the second moments lie a spread above the colour's square, so that both variance rules meet
    positive and clamped differences."""
    rng = np.random.default_rng(seed)
    C, VC, FC = np.zeros((n, 4), f32), np.zeros((n, 4), f32), kept_feedback(n, seed + 1)
    C[:, :3] = rng.random((n, 3), dtype=f32)
    C[:, 3] = (rng.random(n, dtype=f32) * f32(cap)).astype(f32)
    C[rng.random(n) < 0.2, 3] = cap
    C[rng.random(n) < 0.1, 3] = 1.0
    spread = (rng.random((n, 3), dtype=f32) * f32(10.0) ** rng.integers(-8, 0, (n, 3)).astype(f32)).astype(f32)
    spread[rng.random(n) < 0.15] = 0
    VC[:, :3] = C[:, :3] * C[:, :3] + spread
    VC[:, 3] = rng.choice(np.array([1.0, 0.5, 0.25, 0.125, 0.03125], f32), n)
    gone = rng.random(n) < 0.25
    C[gone], VC[gone], FC[gone] = 0, 0, 0
    return C, VC, FC


def extra_plane(n, seed):
    """E [n]: most pixels none, the rest a group or two of three."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0.0, 0.0, 0.0, 3.0, 6.0], f32), n)


# ---- the orbits of tests/test_history_feedback_sim.py: history_moments_ref's (cornell 96 x 54, depth 8, 8 views 3 degrees apart, 1 spp
# per view) with the command line's frame order: lookup (+flag), round, filter, capture (+flag) ----------------------------------------
def run_orbit(views, fns, spp, level, variance, round_fn=None, **dn_opts):
    """views: a list of (camera, S, feature planes).  round_fn(view index, S, feat, C) -> (S, E) or None: the history round between
    the lookup and the filter.  fns: capture, capture_moments, reproject (-> C, VC, FC), denoise (-> image, P), the host functions or
    this module's.  Returns per view (filtered, C, VC, FC, K, VK, P, E)."""
    out = []
    K = VK = FK = kept_cam = None
    for f, (cam, S, feat) in enumerate(views):
        C, VC, FC = (None, None, None) if K is None else fns["reproject"](kept_cam, K, feat, VK, FK)
        E = None
        if round_fn is not None:
            S, E = round_fn(f, S, feat, C)
        filtered, P = fns["denoise"](S, feat, spp, E, C, VC, FC, level, variance, **dn_opts)
        K, VK, FK, kept_cam = fns["capture"](S, feat, spp, E, C), fns["capture_moments"](S, spp, E, C, VC), P, cam
        out.append((filtered, C, VC, FC, K, VK, P, E))
    return out


def host_functions(reject, w, h):
    from cosc_4397_pathtracing_raytracing_project_amd import capi

    def capture(S, feat, spp, E, C):
        return capi.history_capture_host(S, feat, spp, C) if E is None else capi.history_capture_counted_host(S, feat, spp, E, C)

    def capture_moments(S, spp, E, C, VC):
        return capi.history_capture_moments_host(S, spp, C, VC) if E is None else capi.history_capture_moments_counted_host(S, spp, E, C, VC)

    return dict(capture=capture, capture_moments=capture_moments,
                reproject=lambda cam, K, feat, VK, FK: capi.history_reproject_feedback_host(cam, K, feat, reject, VK, FK, w, h),
                denoise=lambda S, feat, spp, E, C, VC, FC, level, variance, **o: capi.history_denoise_feedback_host(
                    S, feat, w, h, spp, E, C, VC, FC, level=level, variance=variance, **o))


# What tests/test_history_feedback_sim.py prints and pins: the MSE of the filtered image at the last view against the 1024-spp frame at
# the last camera, rows L = 1 .. 5, columns variance rule 0, 1; without rounds, with rounds of 3, the camera standing still; and the
# still camera's flicker, the mean squared difference of the filtered outputs of views 7 and 8.  WITHOUT: the same four figures of the
# moments filter without feedback (the first two are history_moments_ref.SIM_FILTERED and history_round_ref's).
SIM_ORBIT = [[0.000756064204, 0.000495588217], [0.000871336844, 0.000543510161], [0.00088412141, 0.000563791677], [0.00088385509, 0.000563776978],
             [0.000883853816, 0.000563776356]]
SIM_ROUNDS = [[0.00078514293, 0.000496055235], [0.00102915305, 0.000563017211], [0.00101592715, 0.00056652759], [0.00101575872, 0.00056660173],
              [0.00101575801, 0.000566601326]]
SIM_STILL = [[0.000616731433, 0.000483048598], [0.00075349824, 0.000574828629], [0.000797620142, 0.000600461926], [0.000797545487, 0.000600396102],
             [0.000797539092, 0.000600390712]]
SIM_FLICKER = [[0.000318220607, 0.000335491456], [0.000323544637, 0.000335625551], [0.000324762502, 0.00033513966], [0.000324753408, 0.000335118489],
               [0.000324753233, 0.000335118372]]
SIM_WITHOUT = [0.000407981136, 0.000186464296, 0.000437550998, 0.000315123297]
# The pairs (L, rule) that are lower than (1, 0) both on the orbit and with the camera standing still: every pair of rule 1.  (1, 1) is
# the lowest of them on both, so it is what the library's defaults are (PT_HISTORY_FEEDBACK_LEVEL, PT_HISTORY_FEEDBACK_VARIANCE).
SIM_BETTER_THAN_DEFAULTS = [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1)]
DEFAULTS = (1, 1)
