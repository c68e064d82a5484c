"""The noise estimate of the blend (include/pt_amd.h pt_history_noise; csrc/pt_history.h noise_value) restated in numpy float32 on
top of history_variance_ref: every operation one IEEE float32 operation on arrays in the order the header states, so W is what the
host twin and the device compute bit for bit.  Also the orbit of tests/test_history_noise_sim.py, the two stopping rules it compares
and the figures it prints."""
import math

import numpy as np

import history_variance_ref as vref
import noise_ref
from history_ref import bits, f32  # noqa: F401  (bits: for the tests)


def history_noise(noise, groups, iters, samples, current=None, current_var=None):
    """(W [n] float32, SSE_blend = the float64 sum of W in pixel order) from the fold's planes [2, n, 4] with their counters M, T and
    the planes C, VC [n, 4] (None: absent)."""
    vb = vref.blend_variance(vref.sample_variance(noise, groups, iters), samples, current, current_var)
    with np.errstate(all="ignore"):
        w = ((vb[:, 0] + vb[:, 1]).astype(f32) + vb[:, 2]).astype(f32)
    return w, float(np.cumsum(w.astype(np.float64))[-1])  # (cumsum adds one after the other; np.sum adds pairwise)


def exact_sum(w):
    """The exactly rounded sum of float32 values (math.fsum), what any summation order is judged against."""
    return math.fsum(float(x) for x in np.asarray(w, f32).reshape(-1))


def psnr_from_sse(sse, pixels):
    """pt_psnr_from_sse on the host, through the library (float32)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    return float(capi.psnr_from_sse(sse, pixels))


# ---- the orbit of tests/test_history_noise_sim.py: history_ref's (cornell 96 x 54, depth 8, 8 views 3 degrees apart); view f renders
# iterations CAP * f + 1 ... in groups of 1 with a fold after each, at most CAP of them -----------------------------------------------
CAP, GROUP = 16, 1
TARGETS = (26.0, 30.0)
MARGIN_DB = 1e-3  # every stop / continue decision of both rules lies at least this far from the target


def first_above(psnrs, target):
    """pt_render_until's rule over the estimates after folds 2, 3, ...: (iterations rendered, the estimates looked at)."""
    for t, p in enumerate(psnrs, start=2):
        if p > target:
            return t, psnrs[:t - 1]
    return len(psnrs) + 1, psnrs


def run_rules(views, truths, reject, w, h, target):
    """Both rules over the orbit at one target.  views: per view (camera, feature planes, [S after t iterations], [noise planes after
    t folds], [the view's SSE_est after t folds]) for t = 1 .. CAP; truths: per view the converged frame at its camera, float64.
    Returns per view a dict: alone / blend (iterations), est_db / actual_db / ratio of the blend at its stop, alone_db, and `looked`,
    every estimate either rule compared with the target."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = w * h
    out = []
    K = VK = kept_cam = None
    for (cam, feat, sums, planes, view_sse), truth in zip(views, truths):
        view_db = [psnr_from_sse(s, n) for s in view_sse[1:]]
        alone, looked = first_above(view_db, target)
        C, VC = (None, None) if K is None else capi.history_reproject_variance_host(kept_cam, K, feat, reject, VK, w, h)
        blend_sse = [capi.history_noise_host(planes[t - 1], t, t, t, C, VC)[1] for t in range(2, len(sums) + 1)]
        blend_db = [psnr_from_sse(s, n) for s in blend_sse]
        stop, looked_blend = first_above(blend_db, target)
        S, noise = sums[stop - 1], planes[stop - 1]
        blend = capi.history_blend_host(S, stop, C)
        actual = float(((np.asarray(blend, np.float64) - truth) ** 2).sum())
        out.append(dict(alone=alone, blend=stop, est_db=blend_db[stop - 2], actual_db=psnr_from_sse(actual, n), ratio=blend_sse[stop - 2] / actual,
                        alone_db=view_db[alone - 2], view_db_at_stop=view_db[stop - 2], looked=list(looked) + list(looked_blend)))
        K, VK, kept_cam = capi.history_capture_host(S, feat, stop, C), capi.history_capture_variance_host(noise, stop, stop, stop, C, VC), cam
    return out


def folded_planes(npix, groups, seed):
    """The fold's planes after every group of a made-up render (noise_ref.random_sums): a list of (planes copy, M, T)."""
    sums, _ = noise_ref.random_sums(npix, groups, seed)
    planes, T, out = noise_ref.new_planes(npix), 0, []
    for M, (n, S) in enumerate(zip(groups, sums), start=1):
        T += n
        noise_ref.fold(S, planes, n, M, T)
        out.append((planes.copy(), M, T))
    return out


def current_planes(n, seed, cap=32.0):
    """C, VC [n, 4] of a lookup that carried most pixels — weights up to the cap, the cap itself for a fifth, rejected pixels (Th = 0)
    all zero — with the variances the estimate branches on: zeros, denormals, huge values, many decades apart."""
    rng = np.random.default_rng(seed)
    C, VC = np.zeros((n, 4), f32), np.zeros((n, 4), f32)
    C[:, :3] = rng.random((n, 3), dtype=f32)
    C[:, 3] = (rng.random(n, dtype=f32) * f32(cap)).astype(f32)
    C[rng.random(n) < 0.2, 3] = cap
    VC[:, :3] = (rng.random((n, 3), dtype=f32) * f32(10.0) ** rng.integers(-12, 1, (n, 3)).astype(f32)).astype(f32)
    kind = rng.integers(0, 8, n) if n > 4 else np.arange(n) % 8
    VC[kind == 0, :3] = 0
    VC[kind == 1, :3] = f32(1e-41)  # denormal
    VC[kind == 2, :3] = f32(3e37)   # huge: the sum of three channels stays below FLT_MAX
    gone = rng.random(n) < 0.25
    C[gone], VC[gone] = 0, 0
    return C, VC


# what tests/test_history_noise_sim.py prints, per target and view 0 .. 7, and the exact build reproduces on the device (the
# iterations): iterations under pt_render_until's rule and under the blend's, the estimated and the actual PSNR of the blend where its
# rule stopped, and the estimated over the actual squared error there (view 0 has no history: the view's own calibration, 0.97 - 0.98;
# with history 1.23 - 2.42: the carried variance reads high, as the header says it must)
SIM_ALONE = {26.0: (12, 12, 12, 12, 11, 11, 11, 11), 30.0: (16, 16, 16, 16, 16, 16, 16, 16)}
SIM_BLEND = {26.0: (12, 2, 2, 2, 2, 2, 2, 2), 30.0: (16, 14, 4, 2, 2, 2, 2, 2)}
SIM_EST_DB = {26.0: (26.2475, 26.3273, 27.0199, 27.7235, 28.0108, 28.3082, 28.5705, 29.1762),
              30.0: (27.4562, 30.0465, 30.0732, 30.1669, 30.1166, 30.1764, 30.25, 30.8189)}
SIM_ACTUAL_DB = {26.0: (26.146, 27.2918, 29.2066, 30.1638, 30.0764, 31.481, 32.0849, 33.0162),
                 30.0: (27.3395, 30.9542, 32.5264, 31.8087, 31.2592, 32.6808, 33.0926, 34.0184)}
SIM_RATIO = {26.0: (0.9769, 1.2487, 1.6545, 1.754, 1.609, 2.0762, 2.2461, 2.4211), 30.0: (0.9735, 1.2325, 1.7592, 1.4594, 1.301, 1.7801, 1.9242, 2.0891)}
