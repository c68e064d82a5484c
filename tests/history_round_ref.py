"""The history round of include/pt_amd.h (pt_history_round: key, select, merge, and the counted forms of blend, capture, the moments
and the moments filter) restated in numpy float32 on top of history_ref and history_moments_ref: every operation one IEEE float32
operation on arrays in the order the header states, so the results are what csrc/pt_history.h and csrc/pt_denoise.h compute bit for
bit.  Also the random planes the host and the GPU tests share, and the orbit of tests/test_history_round_sim.py with its figures."""
import math

import numpy as np

import history_moments_ref as mref
import history_ref as href
from history_ref import bits, f32  # noqa: F401  (bits: for the tests)

MIN_HISTORY = f32(4.0)  # PT_HISTORY_ROUND_MIN_HISTORY


def list_capacity(max_fraction, n):
    """cap = clamp(ceil((double)max_fraction * N), 1, N); 0 = the default 1."""
    f = float(f32(max_fraction)) or 1.0
    return int(min(n, max(1, math.ceil(f * n))))


def keys(feat, current=None, emitter=(), min_history=0.0):
    """The key of every tile pixel as its uint32 bit pattern [n]."""
    feat = np.ascontiguousarray(feat, f32).reshape(3, -1, 4)
    n = feat.shape[1]
    emitter = np.asarray(emitter, np.uint8).reshape(-1)
    mh = MIN_HISTORY if f32(min_history) == 0 else f32(min_history)
    hit = feat[1, :, 3] > 0
    ids = np.ascontiguousarray(feat[2, :, 3]).view(np.int32)
    known = (ids >= 1) & (ids <= emitter.size)
    emits = np.zeros(n, bool)
    emits[known] = emitter[ids[known] - 1] != 0
    Th = np.zeros(n, f32) if current is None else np.ascontiguousarray(current, f32).reshape(-1, 4)[:, 3]
    with np.errstate(all="ignore"):
        d = mh - Th
    assert d.dtype == f32
    key = np.where(d > 0, d, f32(0)).astype(f32)
    key = np.where(hit & known & ~emits, key, f32(0)).astype(f32)
    return key.view(np.uint32)


def select(feat, current=None, emitter=(), min_history=0.0, max_fraction=0.0):
    """(list [m] int32 ascending, fresh, m): the m = min(fresh, cap) fresh pixels with the largest keys, equal keys by the smaller
    tile index."""
    key = keys(feat, current, emitter, min_history)
    cap = list_capacity(max_fraction, key.size)
    fresh = int((key > 0).sum())
    m = min(fresh, cap)
    order = np.lexsort((np.arange(key.size), -key.astype(np.int64)))  # key descending, then index ascending
    lst = np.sort(order[:m]).astype(np.int32)
    assert (key[lst] > 0).all()
    return lst, fresh, m


def merge(rgb_sum, extra, lst, group_sum, group_iters):
    """(S, E) after the merge; the inputs are left alone."""
    S = np.array(rgb_sum, f32).reshape(-1, 3)
    E = np.array(extra, f32).reshape(-1)
    lst = np.asarray(lst, np.int64)
    S[lst] = S[lst] + np.ascontiguousarray(group_sum, f32).reshape(-1, 3)
    E[lst] = E[lst] + f32(group_iters)
    return S, E


def counted(samples, extra):
    """ns [n, 1] = samples + E_p: one float add per pixel, made before anything else."""
    ns = f32(samples) + np.ascontiguousarray(extra, f32).reshape(-1, 1)
    assert ns.dtype == f32
    return ns


def blend(rgb_sum, samples, extra, current=None):
    return href.blend(rgb_sum, counted(samples, extra), current)


def capture(rgb_sum, feat, samples, extra, current=None):
    ns = counted(samples, extra)
    K = href.capture(rgb_sum, feat, 1.0, current)  # K1, K2 do not read the samples
    K[0, :, :3] = href.blend(rgb_sum, ns, current)
    Th = f32(0) if current is None else np.ascontiguousarray(current, f32).reshape(-1, 4)[:, 3]
    K[0, :, 3] = ns[:, 0] + Th
    return K


def capture_moments(rgb_sum, samples, extra, current=None, current_var=None):
    return mref.blend_moments(rgb_sum, counted(samples, extra), current, current_var)


def denoise_moments(rgb_sum, planes, w, rows, samples, extra, current=None, current_var=None, **opts):
    return mref.denoise_moments(rgb_sum, planes, w, rows, counted(samples, extra), current, current_var, **opts)


# ---- inputs the host and the GPU tests share ---------------------------------------------------------------------------------------
SHAPES = [(1, 1), (37, 5), (64, 4), (96, 54)]
NUM_GEOMS = 6
EMITTER = np.array([0, 1, 0, 0, 1, 0], np.uint8)


def random_planes(w, rows, seed=0, weights=(0.0, 1.0, 2.5, 4.0, 7.0, 32.0)):
    """Feature SUM planes [3, n, 4] and a current plane [n, 4]: misses, ids 0 .. NUM_GEOMS + 1 (0 and NUM_GEOMS + 1 lie outside the
    table, EMITTER marks two), and carried weights drawn from a few values, so that runs of equal Th meet every cap."""
    n = w * rows
    rng = np.random.default_rng(1009 * seed + 31 * w + rows)
    feat = rng.standard_normal((3, n, 4)).astype(f32)
    feat[1, :, 3] = np.where(rng.random(n) < 0.15, 0, 1).astype(f32)  # hit flags (sums of 1 spp)
    feat[2, :, 3] = rng.integers(0, NUM_GEOMS + 2, n).astype(np.int32).view(f32)
    C = rng.random((n, 4), dtype=f32)
    C[:, 3] = rng.choice(np.asarray(weights, f32), n)
    return feat, C


def random_image(n, seed=0):
    rng = np.random.default_rng(7919 * seed + n)
    return (rng.random((n, 3), dtype=f32) * f32(3.0)).astype(f32)


def random_extra(n, seed=0):
    """E_p in {0, 2, 4, 8}, about half of them zero."""
    rng = np.random.default_rng(4001 * seed + n)
    return rng.choice(np.asarray([0, 0, 0, 2, 4, 8], f32), n).astype(f32)


# ---- the orbit of tests/test_history_round_sim.py: history_moments_ref's at 1 spp per view (view f renders iteration f + 1), with a
# round of G iterations 1000 + f G + 1 .. after each lookup ---------------------------------------------------------------------------
def run_orbit(views, fns, spp, group_iters, round_samples, min_history=0.0, max_fraction=0.0, emitter=(), **dn_opts):
    """The command line's --denoise-history --history-moments --history-extra order over `views`, a list of (camera, S, feature
    planes): the lookup, the round (select; round_samples(f, list) gives the group sum [m, 3] of the listed pixels; merge), the
    counted blend and filter, the counted capture.  fns: the host functions, or this module's.  Returns per view (blend, filtered
    blend, list, fresh, S, E)."""
    out = []
    K = VK = kept_cam = None
    for f, (cam, S, feat) in enumerate(views):
        n = np.asarray(S).reshape(-1, 3).shape[0]
        C, VC = (None, None) if K is None else fns["reproject_moments"](kept_cam, K, feat, VK)
        E = np.zeros(n, f32)
        lst, fresh, m = fns["select"](feat, C, emitter, min_history, max_fraction)
        lst = lst[:m]
        if m:
            S, E = fns["merge"](S, E, lst, round_samples(f, lst), group_iters)
        blend = fns["blend"](S, spp, E, C)
        filtered = fns["denoise"](S, feat, spp, E, C, VC, **dn_opts)
        K, VK, kept_cam = fns["capture"](S, feat, spp, E, C), fns["capture_moments"](S, spp, E, C, VC), cam
        out.append((blend, filtered, lst, fresh, S, E))
    return out


# what tests/test_history_round_sim.py prints (MSE against the 1024-spp frame at the last camera) and the exact build reproduces on the
# device: rounds of SIM_GROUP iterations with the default min_history — the blend, the filtered blend, the orbit's samples as a multiple
# of the baseline's 8 x 1 spp, the list's length per view; and, for context, the orbit at 2 uniform spp per view without rounds.
# The baseline without rounds is history_moments_ref.SIM_BLEND and SIM_FILTERED.
SIM_GROUP = 3
SIM_ROUND_BLEND, SIM_ROUND_FILTERED, SIM_ROUND_SAMPLES = 0.000869307177, 0.000186464296, 1.19618056
SIM_ROUND_M = [2369, 43, 98, 45, 40, 37, 39, 41]
SIM_2SPP_BLEND, SIM_2SPP_FILTERED = 0.000838322889, 0.000208548492


def host_functions(reject, w, h):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    return dict(reproject_moments=lambda cam, K, feat, VK: capi.history_reproject_moments_host(cam, K, feat, reject, VK, w, h),
                select=lambda feat, C, em, mh, mf: capi.history_select_host(feat, w, h, C, em, mh, mf),
                merge=capi.history_merge_host,
                blend=lambda S, spp, E, C: capi.history_blend_counted_host(S, spp, E, C),
                denoise=lambda S, feat, spp, E, C, VC, **o: capi.history_denoise_moments_counted_host(S, feat, w, h, spp, E, C, VC, **o),
                capture=lambda S, feat, spp, E, C: capi.history_capture_counted_host(S, feat, spp, E, C),
                capture_moments=lambda S, spp, E, C, VC: capi.history_capture_moments_counted_host(S, spp, E, C, VC))


def ref_functions(reject, w, h):
    return dict(reproject_moments=lambda cam, K, feat, VK: mref.reproject_moments(cam, K, feat, reject, VK, w, h),
                select=select, merge=merge, blend=blend,
                denoise=lambda S, feat, spp, E, C, VC, **o: denoise_moments(S, feat, w, h, spp, E, C, VC, **o),
                capture=capture, capture_moments=capture_moments)
