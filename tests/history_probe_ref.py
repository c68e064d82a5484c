"""The history probes of include/pt_amd.h (pt_history_probe_keep / _check: list, keep, gradient, apply) restated in numpy float32:
every operation one IEEE float32 operation on arrays in the order the header states, so the results are what csrc/pt_history.h computes
bit for bit.  Also the inputs the host and the GPU tests share, and the figures of tests/test_history_probe_sim.py."""
import numpy as np

from history_ref import bits, f32  # noqa: F401  (bits: for the tests)

RADIUS, GAIN = 0, f32(0.25)  # PT_HISTORY_PROBE_RADIUS, PT_HISTORY_PROBE_GAIN


def grid(w, rows, phase):
    """(ox, oy, PW, PR)"""
    ox, oy = phase % 3, phase // 3
    return ox, oy, max(0, -((ox - w) // 3)), max(0, -((oy - rows) // 3))


def probe_list(w, rows, phase):
    """The tile pixels of the probes, int32 [P], s = j * PW + i: ascending."""
    ox, oy, PW, PR = grid(w, rows, phase)
    j, i = np.meshgrid(np.arange(PR), np.arange(PW), indexing="ij")
    return ((3 * j + oy) * w + 3 * i + ox).reshape(-1).astype(np.int32)


def ids_of(feat):
    """id_p as the capture reads it: s1.w > 0 ? bits(s2.w) : 0"""
    feat = np.ascontiguousarray(feat, f32).reshape(3, -1, 4)
    return np.where(feat[1, :, 3] > 0, np.ascontiguousarray(feat[2, :, 3]).view(np.int32), 0).astype(np.int32)


def keep(rgb_sum, feat, w, rows, phase):
    """PK [P, 4] = {S_p.xyz, bits(id_p)}"""
    lst = probe_list(w, rows, phase)
    S = np.ascontiguousarray(rgb_sum, f32).reshape(-1, 3)
    PK = np.zeros((lst.size, 4), f32)
    PK[:, :3] = S[lst]
    PK[:, 3] = ids_of(feat)[lst].view(f32)
    return PK


def gradient(kept, group_sum, feat, w, rows, phase, moved=()):
    """(L [P], changed, skipped)"""
    lst = probe_list(w, rows, phase)
    PK = np.ascontiguousarray(kept, f32).reshape(-1, 4)
    Sw = np.ascontiguousarray(group_sum, f32).reshape(-1, 3)
    moved = np.asarray(moved, np.uint8).reshape(-1)
    ids = ids_of(feat)[lst]
    kept_ids = np.ascontiguousarray(PK[:, 3]).view(np.int32)
    known = (ids >= 1) & (ids <= moved.size)
    mv = np.zeros(lst.size, bool)
    mv[known] = moved[ids[known] - 1] != 0
    skip = (ids != kept_ids) | ~known | mv
    with np.errstate(all="ignore"):
        o, wv = PK[:, :3], Sw
        d = (np.abs(wv[:, 0] - o[:, 0]) + np.abs(wv[:, 1] - o[:, 1])) + np.abs(wv[:, 2] - o[:, 2])
        mo = (o[:, 0] + o[:, 1]) + o[:, 2]
        mw = (wv[:, 0] + wv[:, 1]) + wv[:, 2]
        m = np.where(mo > mw, mo, mw)
        lam = np.where(m > 0, d / np.where(m > 0, m, f32(1)), f32(0))
        assert d.dtype == f32 and lam.dtype == f32
        L = np.where(lam < 1, lam, f32(1)).astype(f32)
    L = np.where(skip, f32(-1), L).astype(f32)
    return L, int((L > 0).sum()), int((L < 0).sum())


def lam_pixels(L, w, rows, phase, radius=RADIUS):
    """lam_p [n] before the pixel's own exclusions: the maximum of L over the probes within `radius` cells, starting at +0."""
    _, _, PW, PR = grid(w, rows, phase)
    out = np.zeros((rows, w), f32)
    if PW * PR == 0:
        return out.reshape(-1)
    Lg = np.asarray(L, f32).reshape(PR, PW)
    i0 = np.arange(w) // 3
    j0 = np.arange(rows) // 3
    for dj in range(-radius, radius + 1):
        for di in range(-radius, radius + 1):
            j, i = j0 + dj, i0 + di
            jv, iv = (j >= 0) & (j < PR), (i >= 0) & (i < PW)
            tap = np.zeros((rows, w), f32)
            tap[np.ix_(jv, iv)] = Lg[np.ix_(j[jv], i[iv])]
            out = np.where(tap > out, tap, out)
    return out.reshape(-1)


def eligible(feat, moved=()):
    """The pixels the apply may change: hits with an id inside 1 .. num_geoms whose geom stands still."""
    feat = np.ascontiguousarray(feat, f32).reshape(3, -1, 4)
    moved = np.asarray(moved, np.uint8).reshape(-1)
    ids = np.ascontiguousarray(feat[2, :, 3]).view(np.int32)
    ok = (feat[1, :, 3] > 0) & (ids >= 1) & (ids <= moved.size)
    ok[ok] = moved[ids[ok] - 1] == 0
    return ok


def apply(current, L, feat, w, rows, phase, moved=(), radius=0, gain=0.0):
    """A copy of C [n, 4] with C.w shortened; radius, gain: 0 = the default, radius -1 = 0."""
    radius = RADIUS if radius == 0 else 0 if radius == -1 else radius  # (-1: radius 0)
    gain = GAIN if f32(gain) == 0 else f32(gain)
    C = np.array(current, f32).reshape(-1, 4)
    lam = np.where(eligible(feat, moved), lam_pixels(L, w, rows, phase, radius), f32(0)).astype(f32)
    with np.errstate(all="ignore"):
        g = lam * gain
        g = np.where(g < 1, g, f32(1)).astype(f32)
        scaled = C[:, 3] * (f32(1) - g)
    assert scaled.dtype == f32
    touch = lam > 0
    Cw = np.ascontiguousarray(C[:, 3]).view(np.uint32).copy()
    Cw[touch] = np.ascontiguousarray(scaled).view(np.uint32)[touch]  # (by bits: an untouched pixel keeps its word, a NaN's payload too)
    C[:, 3] = Cw.view(f32)
    return C


# ---- inputs the host and the GPU tests share ---------------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 2), (3, 3), (4, 5), (7, 3), (50, 31), (96, 54)]
NUM_GEOMS = 6
MOVED = np.array([0, 0, 1, 0, 0, 1], np.uint8)


def random_case(w, rows, phase, seed=0):
    """(S [n, 3], feature planes [3, n, 4], PK [P, 4], Sw [P, 3], C [n, 4]).  PK is keep() of an earlier S and an earlier id plane: most
    ids agree with the present ones.  Sw equals PK.xyz for about half of the probes (lam exactly 0); of the rest some differ a little,
    some by more than the larger sum (lam above 1), some pairs are both zero (m == 0) and some hold an infinity or a NaN.  C holds -0
    and NaN words."""
    n = w * rows
    rng = np.random.default_rng(7001 * seed + 97 * w + 13 * rows + phase)
    feat = rng.standard_normal((3, n, 4)).astype(f32)
    feat[1, :, 3] = np.where(rng.random(n) < 0.15, 0, 1).astype(f32)
    feat[2, :, 3] = rng.integers(0, NUM_GEOMS + 2, n).astype(np.int32).view(f32)
    S = (rng.random((n, 3), dtype=f32) * f32(3.0)).astype(f32)
    then = feat.copy()
    flip = rng.random(n) < 0.1
    then[2, flip, 3] = rng.integers(0, NUM_GEOMS + 2, int(flip.sum())).astype(np.int32).view(f32)
    PK = keep(S, then, w, rows, phase)
    P = PK.shape[0]
    Sw = PK[:, :3].copy()
    kind = rng.integers(0, 12, P)
    small = kind == 6
    Sw[small] = Sw[small] * f32(1.0009765625)
    Sw[kind == 7, 1] += f32(0.125)
    big = kind == 8
    Sw[big] = -Sw[big] * f32(3.0)
    zero = kind == 9
    Sw[zero] = 0
    PK[zero, :3] = 0
    Sw[kind == 10, 0] = np.inf
    PK[kind == 11, 2] = np.nan
    C = rng.random((n, 4), dtype=f32)
    C[:, 3] = rng.choice(np.asarray([0.0, 1.0, 2.5, 32.0], f32), n)
    odd = rng.integers(0, 16, n)
    C[odd == 0, 3] = f32(-0.0)
    C[odd == 1, 3] = np.nan
    return S, feat, PK, Sw, C


# ---- the simulation of tests/test_history_probe_sim.py: history_motion_ref's sequence (cornell 96 x 54, depth 8, the sphere diffuse, the
# camera still, the sphere's TRANS x from -2.5 in steps of 0.5 over 8 views of 4 spp, the moments kind with motion) in the command line's
# --history-probe order: lookup, check (from the second view on), keep, round (if asked), resolve, capture -----------------------------
def run_sequence(views, replays, fns, spp, probes=True, extra=0, round_samples=None, emitter=(), radius=0, gain=0.0):
    """views: a list of (camera, geoms, S, feature planes); replays[f]: the previous view's iterations rendered in view f's scene, the
    whole frame's sums [n, 3] (read at the probes' pixels only).  extra: the history round's group, 0 for none; round_samples(f, list)
    gives its group sum.  Returns per view a dict: blend, C (after the check), VC, L, changed, skipped, phase, S, E."""
    out = []
    K = VK = kept_cam = kept_geoms = PK = None
    for f, (cam, geoms, S, feat) in enumerate(views):
        rec = dict(L=None, changed=0, skipped=0, phase=None, moved=None)
        if K is None:
            C = VC = None
        else:
            table, kind = fns["motion_table"](kept_geoms, geoms)
            C, VC = fns["reproject_motion"](kept_cam, K, feat, VK, table, kind)
            if probes:
                phase, moved = (f - 1) % 9, (np.asarray(kind) != 0).astype(np.uint8)
                lst = fns["list"](phase)
                L, changed, skipped = fns["gradient"](PK, np.asarray(replays[f], f32).reshape(-1, 3)[lst], feat, phase, moved)
                C = fns["apply"](C, L, feat, phase, moved, radius, gain)
                rec.update(L=L, changed=changed, skipped=skipped, phase=phase, moved=moved)
        if probes:
            PK = fns["keep"](S, feat, f % 9)
        E = None
        if extra:
            E = np.zeros(np.asarray(S).reshape(-1, 3).shape[0], f32)
            lst, _, m = fns["select"](feat, C, emitter, 0.0, 0.0)
            if m:
                S, E = fns["merge"](S, E, lst[:m], round_samples(f, lst[:m]), extra)
            blend = fns["blend_counted"](S, spp, E, C)
            K, VK = fns["capture_counted"](S, feat, spp, E, C), fns["capture_moments_counted"](S, spp, E, C, VC)
        else:
            blend = fns["blend"](S, spp, C)
            K, VK = fns["capture"](S, feat, spp, C), fns["capture_moments"](S, spp, C, VC)
        kept_cam, kept_geoms = cam, geoms
        rec.update(blend=blend, C=C, VC=VC, S=S, E=E)
        out.append(rec)
    return out


def host_functions(reject, w, h):
    import history_motion_ref as mot
    import history_round_ref as rnd
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    fns = dict(mot.host_functions(reject, w, h))
    r = rnd.host_functions(reject, w, h)
    fns.update(select=r["select"], merge=r["merge"], blend_counted=r["blend"], capture_counted=r["capture"], capture_moments_counted=r["capture_moments"],
               list=lambda phase: capi.history_probe_list_host(w, h, phase),
               keep=lambda S, feat, phase: capi.history_probe_keep_host(S, feat, w, h, phase),
               gradient=lambda PK, Sw, feat, phase, moved: capi.history_probe_gradient_host(PK, Sw, feat, w, h, phase, moved),
               apply=lambda C, L, feat, phase, moved, radius, gain: capi.history_probe_apply_host(C, L, feat, w, h, phase, moved, radius, gain))
    return fns


def ref_functions(reject, w, h):
    import history_motion_ref as mot
    import history_round_ref as rnd
    fns = dict(mot.ref_functions(reject, w, h))
    r = rnd.ref_functions(reject, w, h)
    fns.update(select=r["select"], merge=r["merge"], blend_counted=r["blend"], capture_counted=r["capture"], capture_moments_counted=r["capture_moments"],
               list=lambda phase: probe_list(w, h, phase),
               keep=lambda S, feat, phase: keep(S, feat, w, h, phase),
               gradient=lambda PK, Sw, feat, phase, moved: gradient(PK, Sw, feat, w, h, phase, moved),
               apply=lambda C, L, feat, phase, moved, radius, gain: apply(C, L, feat, w, h, phase, moved, radius, gain))
    return fns


def touched(rec, feat, w, h, radius=RADIUS):
    """The pixels of a checked view whose lam_p > 0 (bool [n])."""
    lam = np.where(eligible(feat, rec["moved"]), lam_pixels(rec["L"], w, h, rec["phase"], radius), f32(0))
    return lam > 0


# what tests/test_history_probe_sim.py prints, at the default radius and gain: per checked view (the second to the eighth) the probes
# changed and skipped and the share of probes with lam == 0; at the last view the pixels off the sphere with lam_p > 0, and the MSE
# against 1024 spp with the probes (and WITHOUT them) over the frame, over those pixels and over the rest; the same with rounds of 3
# extra iterations; and at radius 1 and gain 1 the frame's MSE without and with the rounds, and the round's pixels per view
SIM_CHANGED, SIM_SKIPPED, SIM_TOUCHED = [93, 92, 95, 77, 85, 87, 85], [292, 310, 309, 308, 326, 326, 309], 753
SIM_ZERO = [191, 174, 172, 191, 165, 163, 182]  # of 576 probes per view: a third
SIM_L_SUM = [29.2374131, 31.8937984, 35.3256509, 24.4319146, 26.5135927, 26.5847693, 30.241901]  # the sum of L over the changed probes per view
SIM_FRAME, SIM_FRAME_WITHOUT = 0.000889842768, 0.000882940169  # (without: history_motion_ref.SIM_FRAME_MOTION)
SIM_TOUCHED_MSE, SIM_TOUCHED_MSE_WITHOUT, SIM_REST_MSE, SIM_REST_MSE_WITHOUT = 0.00190067913, 0.0018544954, 0.000718062181, 0.000717834981
SIM_ROUND_FRAME, SIM_ROUND_FRAME_WITHOUT, SIM_ROUND_TOUCHED_MSE, SIM_ROUND_TOUCHED_MSE_WITHOUT = 0.00081863295, 0.000812211853, 0.00174720811, 0.00170124886
SIM_ROUND_REST_MSE, SIM_ROUND_REST_MSE_WITHOUT = 0.000660831754, 0.000661129734
SIM_ROUND_M = [2369, 8, 9, 10, 8, 7, 9, 9]  # the round's pixels per view, with the probes and without
SIM_FULL_FRAME, SIM_FULL_ROUND_FRAME = 0.00283765457, 0.00186975527
SIM_FULL_ROUND_M = [2369, 1457, 1224, 1400, 857, 1059, 925, 1148]
