"""Threshold rounds over the blend (include/pt_amd.h pt_history_round_threshold; csrc/pt_history.h Counts .. capture_counts_pixel,
csrc/pt_denoise.h Form::HistoryAdaptive) restated in numpy float32: every operation below is one IEEE float32 operation on arrays in
the order the header states, so W, NE, the keys, the blend, K, VK and the filtered image are what the host twins and the device compute
bit for bit.  Also the made-up inputs the host and the GPU tests share."""
import numpy as np

import adaptive_threshold_ref as tref
import history_noise_ref as nzref
from denoise_guided_ref import DEFAULT_SIGMA, FLOOR, G, H, dist2, exp32, inv_sigma2
from history_ref import bits, f32, surface  # noqa: F401  (bits: for the tests)

# W x R: not a multiple of 64 or 1024 (six partial sums) | every tap of the stencil meets a border | a row crosses a workgroup
SHAPES = ((97, 61), (3, 2), (257, 5))
CAP = f32(32.0)


def divisors(counts):
    """Tf, Df [n, 1] float32 from counts [n, 2] int32 (T_p, M_p)."""
    counts = np.asarray(counts, np.int32).reshape(-1, 2)
    assert (counts[:, 1] >= 2).all() and (counts[:, 0] >= counts[:, 1]).all()
    Tf = counts[:, 0:1].astype(f32)
    Df = ((counts[:, 1:2] - 1).astype(f32) * Tf).astype(f32)
    return Tf, Df


def planes_or_zero(n, current, current_var):
    C = np.zeros((n, 4), f32) if current is None else np.ascontiguousarray(current, f32).reshape(-1, 4)
    VC = np.zeros((n, 4), f32) if current_var is None else np.ascontiguousarray(current_var, f32).reshape(-1, 4)
    return C, VC


def blend_variance(noise, counts, current=None, current_var=None):
    """vb [n, 3]: per component sample_variance(prev, q, Tf, Df), then blend_variance(vn, Tf, vh, Th)."""
    prev, q = (np.ascontiguousarray(noise, f32).reshape(2, -1, 4)[k][:, :3] for k in range(2))
    Tf, Df = divisors(counts)
    C, VC = planes_or_zero(prev.shape[0], current, current_var)
    Th, vh = C[:, 3:4], VC[:, :3]
    with np.errstate(all="ignore"):
        d = q - (prev * prev) / Tf
        vn = (np.where(d > 0, d, f32(0)) / Df).astype(f32)
        dn = Tf + Th
        wn = Tf / dn
        wh = Th / dn
        return ((wn * wn) * vn + (wh * wh) * vh).astype(f32)


def noise_counts(noise, counts, current=None, current_var=None):
    """Pass A: (W [n], NE [n], vb [n, 4] = {vb.xyz, +0}, SSE_blend = the float64 sum of W in pixel order)."""
    vb = blend_variance(noise, counts, current, current_var)
    Tf, _ = divisors(counts)
    C, _ = planes_or_zero(vb.shape[0], current, None)
    with np.errstate(all="ignore"):
        w = ((vb[:, 0] + vb[:, 1]).astype(f32) + vb[:, 2]).astype(f32)
        ne = (Tf[:, 0] + C[:, 3]).astype(f32)
    vb4 = np.concatenate([vb, np.zeros((vb.shape[0], 1), f32)], axis=1)
    return w, ne, vb4, float(np.cumsum(w.astype(np.float64))[-1])


def keys_blend(w, ne, W, R):
    """Pass B: the uint32 keys [W * R] — adaptive_ref.keys' arithmetic over (W, NE) in place of (plane 0's w, T)."""
    w = np.ascontiguousarray(w, f32).reshape(R, W)
    ne = np.ascontiguousarray(ne, f32).reshape(R, W)
    with np.errstate(all="ignore"):
        s = (w * ne).astype(f32)
        num, den = np.zeros((R, W), f32), np.zeros((R, W), f32)
        for j in (-1, 0, 1):  # rows, outer
            for i in (-1, 0, 1):
                g = f32(G[j + 1] * G[i + 1])
                y0, y1, x0, x1 = max(0, -j), R - max(0, j), max(0, -i), W - max(0, i)  # the pixels whose tap (x + i, y + j) exists
                if y0 >= y1 or x0 >= x1:
                    continue
                tap = s[y0 + j:y1 + j, x0 + i:x1 + i]
                num[y0:y1, x0:x1] = (num[y0:y1, x0:x1] + (g * tap).astype(f32)).astype(f32)
                den[y0:y1, x0:x1] = (den[y0:y1, x0:x1] + g).astype(f32)
        key = ((num / den).astype(f32) / ne).astype(f32)
    out = bits(key).reshape(-1).copy()
    out[np.isnan(key).reshape(-1)] = 0xFFFFFFFF  # a NaN sorts first, whatever its sign and payload
    return out


def select_threshold_blend(noise, counts, W, R, threshold, cap, current=None, current_var=None):
    """(list int32 [m] ascending, above, m): adaptive_threshold_ref.select_threshold's rule on the blend's keys."""
    w, ne, _, _ = noise_counts(noise, counts, current, current_var)
    k = keys_blend(w, ne, W, R)
    is_above = k > np.uint32(tref.threshold_bits(threshold))
    above = int(is_above.sum())
    m = min(above, int(cap))
    if above <= cap:
        return np.flatnonzero(is_above).astype(np.int32), above, m
    order = np.lexsort((np.arange(k.size), -k.astype(np.int64)))  # key descending, then index ascending
    return np.sort(order[:m]).astype(np.int32), above, m


def blend(rgb_sum, counts, current=None):
    """c_k = blend_component(S_k, Tf_p, C.k, C.w): [n, 3]."""
    S = np.ascontiguousarray(rgb_sum, f32).reshape(-1, 3)
    Tf, _ = divisors(counts)
    C, _ = planes_or_zero(S.shape[0], current, None)
    with np.errstate(all="ignore"):
        m = C[:, :3] * C[:, 3:4]
        a = S + m
        d = Tf + C[:, 3:4]
        return (a / d).astype(f32)


def capture(rgb_sum, feat, noise, counts, current=None, current_var=None):
    """(K [3, n, 4], VK [n, 4]): K0 = {blend, Tf_p + Th}, K1 = {position, id}, K2 = {normal, 0}, VK = {vb.xyz, +0}."""
    S = np.ascontiguousarray(rgb_sum, f32).reshape(-1, 3)
    n_pix = S.shape[0]
    _, ne, vb4, _ = noise_counts(noise, counts, current, current_var)
    _, n, p, ids = surface(feat)
    K = np.zeros((3, n_pix, 4), f32)
    K[0, :, :3] = blend(S, counts, current)
    K[0, :, 3] = ne
    K[1, :, :3] = p
    K[1, :, 3] = ids.view(f32)
    K[2, :, :3] = n
    return K, vb4


def denoise(rgb_sum, planes, noise, counts, w, rows, current=None, current_var=None, levels=0, sigma_color=0.0, sigma_normal=0.0, sigma_position=0.0,
            keep_albedo=False, stats=None):
    """pt_history_denoise_adaptive: pt_history_denoise's prepare with the counts of every pixel — the colour is the blend, the variance the
    blend's, NE in the position buffer's spare word — then pt_denoise_adaptive's per-sample prefilter (over var_raw * NE), levels and
    finish.  `stats` receives var_raw and var_0."""
    levels = levels or 5
    s0, s1, s2 = (np.asarray(planes, f32).reshape(3, rows, w, 4)[k] for k in range(3))
    inv_c, inv_n, inv_p = (inv_sigma2(s, d) for s, d in zip((sigma_color, sigma_normal, sigma_position), DEFAULT_SIGMA))
    hit = s1[..., 3] > 0
    den = np.where(hit, s1[..., 3], f32(1))[..., None]
    zero = np.zeros((rows, w, 3), f32)
    n = np.where(hit[..., None], s0[..., :3] / den, zero)
    a = np.where(hit[..., None], s1[..., :3] / den, zero)
    p = np.where(hit[..., None], s2[..., :3] / den, zero)
    c = blend(rgb_sum, counts, current).reshape(rows, w, 3)
    demod = (a > 0) & (not keep_albedo)
    safe_a = np.where(demod, a, f32(1))
    Tf, _ = divisors(counts)
    C, _ = planes_or_zero(w * rows, current, None)
    with np.errstate(all="ignore"):
        ne = (Tf[:, 0] + C[:, 3]).astype(f32).reshape(rows, w)
        c = np.where(demod, c / safe_a, c)
        v = blend_variance(noise, counts, current, current_var).reshape(rows, w, 3)
        v = np.where(demod, v / (safe_a * safe_a), v)
        var_raw = (v[..., 0] + v[..., 1]) + v[..., 2]
    assert c.dtype == f32 and var_raw.dtype == f32 and ne.dtype == f32
    ys, xs = np.mgrid[0:rows, 0:w]

    def tap(dy, dx):
        y, x = ys + dy, xs + dx
        inside = (y >= 0) & (y < rows) & (x >= 0) & (x < w)
        yc, xc = np.clip(y, 0, rows - 1), np.clip(x, 0, w - 1)
        return yc, xc, inside & (hit[yc, xc] == hit)

    num, gsum = np.zeros((rows, w), f32), np.zeros((rows, w), f32)
    with np.errstate(all="ignore"):
        for j in range(-1, 2):
            for i in range(-1, 2):
                yc, xc, take = tap(j, i)
                g = G[j + 1] * G[i + 1]
                s = var_raw[yc, xc] * ne[yc, xc]
                num = num + np.where(take, g * s, f32(0))
                gsum = gsum + np.where(take, g, f32(0))
        var = (num / gsum) / ne
    var_0 = var
    assert var.dtype == f32
    for l in range(levels):  # the guided form's levels
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


# ---- the made-up inputs -------------------------------------------------------------------------------------------------------------
def random_counts(n, seed=0):
    """counts [n, 2] int32: T_p over 2 .. 40, M_p over 2 .. T_p; both ends of both ranges occur where n allows."""
    rng = np.random.default_rng(77 * n + seed)
    c = np.empty((n, 2), np.int32)
    c[:, 0] = rng.integers(2, 41, n)
    c[:, 1] = rng.integers(2, c[:, 0] + 1)
    if n >= 4:
        c[0], c[1], c[2], c[3] = (2, 2), (40, 2), (40, 40), (17, 3)
    return c


def uniform_counts(n, T, M):
    c = np.empty((n, 2), np.int32)
    c[:, 0], c[:, 1] = T, M
    return c


def noise_planes(counts, seed=0):
    """The planes [2, n, 4] a render with those counts could have left: prev = S (sums of T_p samples), q >= S^2 / T up to rounding;
    every fifth pixel has q = S^2 / T in float32 (zero or rounding-sized variance, some clamped), every eleventh is black (all zero).
    Returns (planes, S [n, 3])."""
    n = counts.shape[0]
    rng = np.random.default_rng(13 * n + seed)
    Tf = counts[:, 0:1].astype(f32)
    S = (rng.random((n, 3), dtype=f32) * f32(2) * Tf).astype(f32)
    S[np.arange(n) % 11 == 10] = 0
    with np.errstate(all="ignore"):
        floor = ((S * S) / Tf).astype(f32)
        q = (floor * (f32(1) + rng.random((n, 3), dtype=f32) * f32(0.5))).astype(f32)
    flat = np.arange(n) % 5 == 4
    q[flat] = floor[flat]
    planes = np.zeros((2, n, 4), f32)
    planes[0, :, :3], planes[1, :, :3] = S, q
    w, _, _, _ = noise_counts(planes, counts)
    planes[0, :, 3] = w  # what a fold or a merge leaves in the spare word: the view's own estimate
    return planes, S


def current_planes(n, seed=0):
    """history_noise_ref.current_planes (Th = 0 beside Th = cap, zero, denormal and huge variances), and — where the tile has the room —
    a NaN and an infinity in VC at two carried pixels."""
    C, VC = nzref.current_planes(n, seed, float(CAP))
    carried = np.flatnonzero(C[:, 3] > 0)
    if carried.size >= 2 and n > 6:
        VC[carried[0], 1] = np.nan
        VC[carried[-1], 0] = np.inf
    return C, VC


def thresholds(noise, counts, W, R, current, current_var):
    """{name: threshold}: 0; below the smallest positive key; between two keys; above the largest finite key.  (A threshold whose
    square IS a key: tie_planes.)"""
    w, ne, _, _ = noise_counts(noise, counts, current, current_var)
    k = keys_blend(w, ne, W, R)
    vals = np.unique(k[k < 0x7F800000]).view(f32)
    pos = vals[vals > 0]
    out = {"zero": 0.0}
    if pos.size:
        out["below"] = float(np.sqrt(pos[0].astype(np.float64)) * 0.5)
        out["past"] = float(np.sqrt(pos[-1].astype(np.float64)) * 2.0 + 1.0)
        if pos.size > 1:
            lo, hi = pos[pos.size // 2 - 1], pos[pos.size // 2]
            between = f32(np.sqrt((lo.astype(np.float64) + hi.astype(np.float64)) / 2))
            if lo <= f32(between * between) < hi:
                out["between"] = float(between)
    return out


def tie_planes(W, R):
    """Inputs whose keys are exact.  Every pixel has (T, M) = (4, 2), prev = 4 and q = 10 per channel: vn = (10 - 16 / 4) / 4 = 1.5; with
    Th = 4 and vh = 1.5 the weights are 1/2 each, vb = 0.75 per channel, W = 2.25 and NE = 8.  s = W * NE is one value, the prefilter's
    weights are dyadic, so num / den is s and every key is 2.25 = 1.5^2 exactly: a threshold of 1.5 meets the keys, and equal is not
    above.  Every 29th pixel is hotter (q = 100), which lifts it and its neighbours above.  Returns (noise, counts, C, VC, threshold)."""
    n = W * R
    counts = uniform_counts(n, 4, 2)
    noise = np.zeros((2, n, 4), f32)
    noise[0, :, :3] = f32(4.0)
    noise[1, :, :3] = f32(10.0)
    noise[1, np.arange(n) % 29 == 7, :3] = f32(100.0)
    C, VC = np.zeros((n, 4), f32), np.zeros((n, 4), f32)
    C[:, :3], C[:, 3] = f32(1.0), f32(4.0)
    VC[:, :3] = f32(1.5)
    noise[0, :, 3] = noise_counts(noise, counts)[0]
    return noise, counts, C, VC, 1.5


def caps(n):
    return sorted({1, -(-n // 4), n})


# ---- the orbit of tests/test_history_threshold_sim.py: history_ref's (cornell 96 x 54, depth 8, 8 views 3 degrees apart); view f has the
# iteration numbers ORBIT_CAP * f + 1 ... in groups of ORBIT_GROUP: two uniform groups with a fold after each, then threshold rounds -------
ORBIT_CAP, ORBIT_GROUP, ORBIT_MIN_PIXELS, ORBIT_FRACTION = 16, 2, 5, 1.0


def oracle_view(ob, path, res, f, threads):
    """What the rounds of view f can draw on: the SUM image after each of the two uniform groups (accumulated sample by sample, as the
    renderer's image is) and, for every later group of iteration numbers, the frame's group sum from zero (as the worker's is)."""
    first = f * ORBIT_CAP + 1
    ob.load_scene(path, res=res)
    u1 = ob.render(first, ORBIT_GROUP, variant=ob.RETIRE, nthreads=threads)
    u2 = ob.render(first + ORBIT_GROUP, ORBIT_GROUP, variant=ob.RETIRE, nthreads=threads, accum=u1.copy())
    groups = [ob.render(first + g * ORBIT_GROUP, ORBIT_GROUP, variant=ob.RETIRE, nthreads=threads) for g in range(2, ORBIT_CAP // ORBIT_GROUP)]
    return u1, u2, groups


def simulate_view(capi, w, h, uniform, groups, threshold, current=None, current_var=None, blend_rule=True):
    """pt_render_threshold (blend_rule False) or pt_history_render_threshold over one view through the library's host functions:
    (S, noise planes, counts, iteration numbers used, pixel-samples, pixels above at the last count, rounds)."""
    import noise_ref
    n = w * h
    planes = noise_ref.new_planes(n)
    for g, S in enumerate(uniform, start=1):
        capi.noise_fold_host(S, planes, ORBIT_GROUP, g, g * ORBIT_GROUP)
    S = np.ascontiguousarray(uniform[-1], f32).copy()
    counts = uniform_counts(n, 2 * ORBIT_GROUP, 2)
    used, samples, above, rounds = 2 * ORBIT_GROUP, 2 * ORBIT_GROUP * n, -1, 0
    cap = n  # max_fraction 1
    for B in groups:
        if blend_rule:
            lst, above, m = capi.history_select_threshold_blend_host(planes, counts, w, h, threshold, cap, current, current_var)
        else:
            lst, above, m = capi.adaptive_select_threshold_host(planes, counts, w, h, threshold, cap)
        if above <= ORBIT_MIN_PIXELS:
            break
        capi.adaptive_merge_host(S, planes, counts, lst, B[lst], ORBIT_GROUP)
        used += ORBIT_GROUP
        samples += ORBIT_GROUP * m
        rounds += 1
    return S, planes, counts, used, samples, above, rounds


def run_orbit_rules(capi, views, truths, reject, w, h, threshold, **dn_opts):
    """Both rules over the orbit.  views: per view (camera, feature planes, [S after uniform group 1, 2], [group sums of the later
    groups]); truths: per view the converged frame at its camera, float64.  The rule without history renders every view on its own; the
    blend's rule carries K and VK from view to view.  Returns per view a dict of both rules' figures."""
    n = w * h
    out = []
    K = VK = kept_cam = None
    for (cam, feat, uniform, groups), truth in zip(views, truths):
        _, _, _, alone_used, alone_samples, alone_above, alone_rounds = simulate_view(capi, w, h, uniform, groups, threshold, blend_rule=False)
        C, VC = (None, None) if K is None else capi.history_reproject_variance_host(kept_cam, K, feat, reject, VK, w, h)
        S, planes, counts, used, samples, above, rounds = simulate_view(capi, w, h, uniform, groups, threshold, C, VC)
        wp, ne, _, sse = capi.history_noise_adaptive_host(planes, counts, C, VC)
        blend_img = capi.history_blend_adaptive_host(S, counts, C)
        filtered = capi.history_denoise_adaptive_host(S, feat, planes, counts, w, h, C, VC, **dn_opts)
        err2 = ((np.asarray(blend_img, np.float64) - truth) ** 2).sum(axis=1)
        finished = keys_blend(wp, ne, w, h) <= np.uint32(tref.threshold_bits(threshold))
        out.append(dict(alone_used=alone_used, alone_samples=alone_samples, alone_above=alone_above, alone_rounds=alone_rounds, used=used, samples=samples,
                        above=above, rounds=rounds, mse=float(err2.sum() / (3 * n)), mse_filtered=float(((np.asarray(filtered, np.float64) - truth) ** 2).sum() / (3 * n)),
                        finished=int(finished.sum()), finished_over=float((err2[finished] > float(threshold) ** 2).mean()) if finished.any() else 0.0,
                        ratio=float(sse / err2.sum())))
        K, VK = capi.history_capture_adaptive_host(S, feat, planes, counts, C, VC)
        kept_cam = cam
    return out


# E of the orbit: a scan over 0.1, 0.15, 0.2, 0.25, 0.3, 0.5 at this cap — at 0.2 and below no view on its own ends before its 16 iteration
# numbers are used, at 0.3 and above the rounds handle a few dozen pixels; at 0.25 (thr = 1/16 exactly) view 0 uses its whole cap and
# views 1 .. 7 on their own end below it.  What tests/test_history_threshold_sim.py prints per view 0 .. 7 and the exact build reproduces
# on the device: iteration numbers used and pixel-samples under pt_render_threshold's rule and under the blend's; and of the last view
# the mean squared error of the blend and of the filtered blend against 1024 spp.
SIM_E = 0.25
SIM_ALONE_USED = (16, 12, 14, 14, 12, 12, 12, 12)
SIM_ALONE_SAMPLES = (22514, 22268, 22592, 22382, 22364, 22520, 22224, 22226)
SIM_BLEND_USED = (16, 6, 10, 8, 10, 6, 8, 6)
SIM_BLEND_SAMPLES = (22514, 20806, 20810, 20772, 20808, 20762, 20788, 20754)
SIM_LAST_MSE, SIM_LAST_MSE_FILTERED = 4.214087e-4, 1.438650e-4
# recorded, not bounded: the share of finished pixels (key <= thr) whose actual error exceeds E, and the estimated over the actual squared
# error of the blend (view 0 has no history: the view's own calibration; with history the carried variance reads high)
SIM_FINISHED_OVER = (0.0554, 0.0145, 0.0044, 0.0035, 0.0021, 0.0031, 0.0012, 0.0025)
SIM_RATIO = (0.8716, 1.2284, 1.5972, 1.6444, 1.8975, 1.7367, 2.1307, 1.9315)
