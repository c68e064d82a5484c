"""The variance-guided filter with per-pixel sample counts on the host (pt_denoise_adaptive_host: csrc/pt_denoise.h, the bodies
the HIP kernels run too) against the numpy restatement tests/denoise_adaptive_ref.py, bit for bit; its prepared variance against
the merge's own; and the uniform state against pt_denoise_guided_host.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref
import denoise_adaptive_ref as aref
import denoise_guided_ref as gref
import denoise_ref as ref
import noise_ref
from denoise_ref import FRAMES, bits, f32

GROUPS, ITERS = 3, 7  # of the made-up render behind the noise planes; the counts are made up separately
OPTIONS = {
    "defaults": dict(),
    "levels8": dict(levels=8),
    "levels3_keep_albedo": dict(levels=3, keep_albedo=True),
    "colour_off": dict(sigma_color=-1.0),
    "own_colour_normal_off": dict(sigma_color=3.0, sigma_normal=-1.0),
}
_FRAMES = {}


def frame(w, rows):
    """(SUM image, feature SUM planes, noise planes, counts) of a frame no renderer would produce; shared, read-only."""
    if (w, rows) not in _FRAMES:
        _, planes = ref.random_frame(w, rows, ITERS)
        noise = gref.random_noise_planes(w, rows, GROUPS, ITERS)
        rgb = np.ascontiguousarray(noise[0, :, :3])  # prev == S, as the fold and the merge leave them
        counts = aref.random_counts(w, rows)
        for a in (rgb, planes, noise, counts):
            a.setflags(write=False)
        _FRAMES[(w, rows)] = (rgb, planes, noise, counts)
    return _FRAMES[(w, rows)]


def same(got, want, what):
    got, want = np.asarray(got).reshape(len(want), -1), np.asarray(want).reshape(len(want), -1)
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:2]], want[bad[:2]])


def pow2(t):
    return (t & (t - 1)) == 0


# ---- 1: the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(OPTIONS))
@pytest.mark.parametrize("w,rows", FRAMES)
def test_host_equals_restatement(w, rows, name):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rgb, planes, noise, counts = frame(w, rows)
    stats = {}
    want = aref.denoise_adaptive(rgb, planes, noise, counts, w, rows, stats=stats, **OPTIONS[name])
    if w * rows > 1:  # (one pixel has one count; the three larger frames carry the conditions)
        hits, misses, _ = ref.frame_properties(rgb, planes)
        T = counts[:, 0]
        assert hits > 0 and misses > 0
        assert (stats["var_raw"] == 0).any() and (stats["var_raw"] > 0).any()
        assert np.unique(T).size >= 3 and pow2(T).any() and (~pow2(T)).any()
        assert counts[:, 1].min() >= 2 and counts[:, 1].max() <= 6 and (T >= counts[:, 1]).all()
    got = capi.denoise_adaptive_host(rgb, planes, noise, counts, w, rows, **OPTIONS[name])
    assert np.isfinite(want).all()
    same(got, want, (w, rows, name))


@pytest.mark.parametrize("keep_albedo", [False, True])
@pytest.mark.parametrize("w,rows", FRAMES)
def test_variances_equal_restatement(w, rows, keep_albedo):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rgb, planes, noise, counts = frame(w, rows)
    stats = {}
    aref.denoise_adaptive(rgb, planes, noise, counts, w, rows, levels=1, keep_albedo=keep_albedo, stats=stats)
    raw, pre = capi.denoise_adaptive_variance_host(rgb, planes, noise, counts, w, rows, keep_albedo=keep_albedo)
    same(raw, stats["var_raw"], "var_raw")
    same(pre, stats["var_0"], "var_0")
    assert w * rows == 1 or (bits(pre) != bits(raw)).any()


# ---- 2: the prepared variance is the merge's own ------------------------------------------------------------------------------
@pytest.mark.parametrize("w,rows", [(33, 9), (97, 11)])
def test_prepared_variance_is_the_merges_own(w, rows):
    """Two folded groups of 3 and three rounds of 3 over a quarter of the pixels (adaptive_ref.select / merge over made-up group
    sums): (v_x + v_y) + v_z of the prepare step, without demodulation, equals the w plane bit for bit, for the merged pixels
    (the merge's v_k) and for the pixels no round has touched (the fold's)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = w * rows
    sums, _ = noise_ref.random_sums(n, (3, 3), 77 * w + rows)
    noise, T = noise_ref.new_planes(n), 0
    for M, S in enumerate(sums, start=1):
        T += 3
        noise_ref.fold(S, noise, 3, M, T)
    S = sums[-1].copy()
    counts = adaptive_ref.uniform_counts(n, T, 2)
    rng = np.random.default_rng(w + rows)
    m = adaptive_ref.list_length(0.25, n)
    for _ in range(3):
        lst = adaptive_ref.select(noise[0, :, 3], w, rows, counts, m)
        Sw = (rng.exponential(1.0, (m, 3)) * rng.uniform(0, 2, (m, 3)) * 3).astype(f32)
        adaptive_ref.merge(S, noise, counts, lst, Sw, 3)
    assert np.unique(counts[:, 0]).size >= 3 and (counts[:, 0] == T).any()
    assert np.array_equal(bits(S), bits(noise[0, :, :3]))  # prev == S
    _, planes = ref.random_frame(w, rows, 4)
    raw, _ = capi.denoise_adaptive_variance_host(S, planes, noise, counts, w, rows, keep_albedo=True)
    assert (noise[0, :, 3] > 0).sum() > n // 4
    same(raw, noise[0, :, 3], (w, rows))


# ---- 3, 4: the uniform state ------------------------------------------------------------------------------------------------------
def uniform_frame(w, rows, groups, iters):
    """frame() for a uniform render of `iters` iterations in `groups` groups, with the pixels whose variance is tiny (random_sums'
    classes around 1e-20 and 1e-30) made all-zero pixels, so that no product of the two prefilters is subnormal."""
    _, planes = ref.random_frame(w, rows, iters)
    noise = gref.random_noise_planes(w, rows, groups, iters)
    tiny = (noise[0, :, 3] > 0) & (noise[0, :, 3] < 1e-12)
    noise[:, tiny, :] = 0
    return np.ascontiguousarray(noise[0, :, :3]), planes, noise


@pytest.mark.parametrize("opts", [dict(), dict(keep_albedo=True, levels=3)])
@pytest.mark.parametrize("w,rows", FRAMES)
def test_uniform_power_of_two_is_the_guided_filter(w, rows, opts):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    T, M = 8, 4
    rgb, planes, noise = uniform_frame(w, rows, M, T)
    counts = aref.uniform_counts(w * rows, T, M)
    raw, pre = capi.denoise_adaptive_variance_host(rgb, planes, noise, counts, w, rows, **opts)
    assert (raw[raw > 0] >= 2.0 ** -100).all()
    assert w * rows == 1 or ((raw > 0).any() and (raw == 0).any())
    graw, gpre = capi.denoise_guided_variance_host(rgb, planes, noise, w, rows, M, T, **opts)
    same(raw, graw, "var_raw")
    same(pre, gpre, "var_0")
    same(capi.denoise_adaptive_host(rgb, planes, noise, counts, w, rows, **opts), capi.denoise_guided_host(rgb, planes, noise, w, rows, M, T, **opts),
         (w, rows, opts))


@pytest.mark.parametrize("w,rows", FRAMES)
def test_uniform_other_counts_agree_to_a_few_roundings(w, rows):
    """T = 7, M = 3: s = var_raw * Tf, g * s, the nine additions, num / den and the division by Tf are fewer than 32 roundings of
    a sum of non-negative terms, against the guided prefilter's own: the two var_0 agree to 32 * 2^-24 relative wherever both are
    normal numbers."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    T, M = 7, 3
    rgb, planes, noise = uniform_frame(w, rows, M, T)
    counts = aref.uniform_counts(w * rows, T, M)
    same(capi.denoise_adaptive_host(rgb, planes, noise, counts, w, rows), aref.denoise_adaptive(rgb, planes, noise, counts, w, rows), (w, rows))
    raw, pre = capi.denoise_adaptive_variance_host(rgb, planes, noise, counts, w, rows)
    graw, gpre = capi.denoise_guided_variance_host(rgb, planes, noise, w, rows, M, T)
    same(raw, graw, "var_raw")
    tiny = np.finfo(f32).tiny
    normal = (pre >= tiny) & (gpre >= tiny)
    assert w * rows == 1 or normal.any()
    assert ((pre == 0) == (gpre == 0)).all()
    rel = np.abs(pre[normal].astype(np.float64) - gpre[normal]) / gpre[normal]
    print("pixels compared", int(normal.sum()), "differing", int((bits(pre) != bits(gpre)).sum()), "largest relative difference", rel.max() if rel.size else 0.0)
    assert (rel <= 32 * 2.0 ** -24).all()


# ---- 5: refusals ------------------------------------------------------------------------------------------------------------------
def bad_counts(pixel, T, M):
    c = np.array(frame(5, 3)[3])
    c[pixel] = (T, M)
    return c


@pytest.mark.parametrize("fn", ["denoise_adaptive_host", "denoise_adaptive_variance_host"])
@pytest.mark.parametrize("counts,opts,match", [
    (bad_counts(7, 5, 1), dict(), "pixel 7 .*M = 1"), (bad_counts(11, 2, 3), dict(), "pixel 11 .*T = 2"), (bad_counts(0, 0, 0), dict(), "pixel 0 "),
    (None, dict(levels=9), "levels"), (None, dict(levels=-1), "levels"), (None, dict(sigma_color=float("nan")), "sigma"),
    (None, dict(sigma_position=float("inf")), "sigma"),
])
def test_refusals(fn, counts, opts, match):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rgb, planes, noise, good = frame(5, 3)
    with pytest.raises(capi.PtError, match="pt_" + fn + ": .*" + match):
        getattr(capi, fn)(rgb, planes, noise, good if counts is None else counts, 5, 3, **opts)


@pytest.mark.parametrize("null", range(5))
def test_null_pointers_are_refused(null):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rgb, planes, noise, counts = frame(5, 3)
    out = np.empty((15, 3), f32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    args = [rgb.ctypes.data_as(fp), planes.ctypes.data_as(fp), noise.ctypes.data_as(fp), counts.ctypes.data_as(ip), None, out.ctypes.data_as(fp)]
    args[null if null < 4 else 5] = None
    assert capi.lib().pt_denoise_adaptive_host(5, 3, *args) != 0
    msg = capi.lib().pt_last_error().decode()
    assert msg.startswith("pt_denoise_adaptive_host: ") and "null" in msg, msg


def test_sizes_are_checked():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rgb, planes, noise, counts = frame(5, 3)
    with pytest.raises(capi.PtError):
        capi.denoise_adaptive_host(rgb, planes, noise, counts, 5, 4)
    with pytest.raises(capi.PtError):
        capi.denoise_adaptive_host(rgb, planes, noise, counts[:-1], 5, 3)
    with pytest.raises(capi.PtError, match="pt_denoise_adaptive_host: .*0 x 3"):
        capi.denoise_adaptive_host(rgb[:0], planes[:, :0], noise[:, :0], counts[:0], 0, 3)


def test_sigma_color_zero_is_eight():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rgb, planes, noise, counts = frame(33, 9)
    default = capi.denoise_adaptive_host(rgb, planes, noise, counts, 33, 9)
    same(capi.denoise_adaptive_host(rgb, planes, noise, counts, 33, 9, sigma_color=8.0, levels=5), default, "8")
    assert (bits(capi.denoise_adaptive_host(rgb, planes, noise, counts, 33, 9, sigma_color=4.0)) != bits(default)).any()
