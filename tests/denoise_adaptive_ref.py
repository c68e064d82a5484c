"""numpy restatement of the variance-guided filter with per-pixel sample counts as include/pt_amd.h specifies it
(pt_denoise_adaptive), the reference of tests/test_denoise_adaptive_host.py and tests/test_gpu_denoise_adaptive.py.  Like
denoise_guided_ref, whose exp32, dist2, H, G and FLOOR it uses: every operand np.float32, every operation a separate numpy
operation in the stated order, vectorised over the frame, one pass per tap (rows outer, columns inner), a skipped tap adds +0.
Comparisons against it are on bit patterns."""
import numpy as np

from denoise_guided_ref import DEFAULT_SIGMA, FLOOR, G, H, bits, dist2, exp32, inv_sigma2  # noqa: F401  (bits: for the tests)

f32 = np.float32


def denoise_adaptive(rgb_sum, planes, noise, counts, w, rows, levels=0, sigma_color=0.0, sigma_normal=0.0, sigma_position=0.0,
                     keep_albedo=False, stats=None):
    """rgb_sum [w*rows, 3] SUM image, planes [3, w*rows, 4] feature SUM planes, noise [2, w*rows, 4] the planes the folds and
    merges left, counts [w*rows, 2] int32 (T_p, M_p) -> averaged radiance [w*rows, 3].  `stats` (a dict) receives var_raw, var_0
    and var (the variance after the last level), [w*rows] each, and 'cut' as in denoise_ref."""
    levels = levels or 5
    S = np.asarray(rgb_sum, f32).reshape(rows, w, 3)
    s0, s1, s2 = (np.asarray(planes, f32).reshape(3, rows, w, 4)[k] for k in range(3))
    prev, q = (np.asarray(noise, f32).reshape(2, rows, w, 4)[k][..., :3] for k in range(2))
    counts = np.asarray(counts, np.int32).reshape(rows, w, 2)
    inv_c, inv_n, inv_p = (inv_sigma2(s, d) for s, d in zip((sigma_color, sigma_normal, sigma_position), DEFAULT_SIGMA))
    assert (counts[..., 1] >= 2).all() and (counts[..., 0] >= counts[..., 1]).all()
    Tf = counts[..., 0].astype(f32)
    Df = (counts[..., 1] - 1).astype(f32) * Tf
    assert Tf.dtype == f32 and Df.dtype == f32
    # prepare
    hit = s1[..., 3] > 0
    den = np.where(hit, s1[..., 3], f32(1))[..., None]
    zero = np.zeros((rows, w, 3), f32)
    n = np.where(hit[..., None], s0[..., :3] / den, zero)
    a = np.where(hit[..., None], s1[..., :3] / den, zero)
    p = np.where(hit[..., None], s2[..., :3] / den, zero)
    c = S / Tf[..., None]
    demod = (a > 0) & (not keep_albedo)
    safe_a = np.where(demod, a, f32(1))
    c = np.where(demod, c / safe_a, c)
    with np.errstate(under="ignore"):
        d = q - (prev * prev) / Tf[..., None]
        v = np.where(d > 0, d, f32(0)) / Df[..., None]
        v = np.where(demod, v / (safe_a * safe_a), v)
    var_raw = (v[..., 0] + v[..., 1]) + v[..., 2]
    assert c.dtype == f32 and var_raw.dtype == f32
    ys, xs = np.mgrid[0:rows, 0:w]

    def tap(dy, dx):
        y, x = ys + dy, xs + dx
        inside = (y >= 0) & (y < rows) & (x >= 0) & (x < w)
        yc, xc = np.clip(y, 0, rows - 1), np.clip(x, 0, w - 1)
        return yc, xc, inside & (hit[yc, xc] == hit)

    # variance prefilter, over the per-sample variance
    num, gsum = np.zeros((rows, w), f32), np.zeros((rows, w), f32)
    with np.errstate(under="ignore", over="ignore"):
        for j in range(-1, 2):
            for i in range(-1, 2):
                yc, xc, take = tap(j, i)
                g = G[j + 1] * G[i + 1]
                s = var_raw[yc, xc] * Tf[yc, xc]
                num = num + np.where(take, g * s, f32(0))
                gsum = gsum + np.where(take, g, f32(0))
        var = (num / gsum) / Tf
    var_0 = var
    assert var.dtype == f32
    cut = 0
    for l in range(levels):  # the guided form's levels
        s = 1 << l
        with np.errstate(under="ignore", over="ignore"):
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
                    cut += int((take & (-e < f32(-80))).sum())
                    acc = acc + wgt[..., None] * cq
                    wsum = wsum + wgt
                    vsum = vsum + (wgt * wgt) * var[yc, xc]
            c = acc / wsum[..., None]
            var = vsum / (wsum * wsum)
        assert c.dtype == f32 and var.dtype == f32
    if stats is not None:
        stats.update(cut=cut, var_raw=var_raw.reshape(-1), var_0=var_0.reshape(-1), var=var.reshape(-1))
    return np.where(demod, c * a, c).reshape(-1, 3)


def random_counts(w, rows, seed=0):
    """Heterogeneous counts [w*rows, 2] int32 (T_p, M_p): M_p in 2 .. 6, T_p >= M_p; about a third of the pixels have a power
    of two for T_p (8, 16, 32), the others M_p + 0 .. 29, powers of two or not as they fall."""
    n = w * rows
    rng = np.random.default_rng(500 * w + 7 * rows + seed)
    counts = np.empty((n, 2), np.int32)
    counts[:, 1] = rng.integers(2, 7, n)
    counts[:, 0] = counts[:, 1] + rng.integers(0, 30, n)
    pow2 = rng.random(n) < 1 / 3
    counts[pow2, 0] = rng.choice(np.array([8, 16, 32], np.int32), int(pow2.sum()))
    return counts


def uniform_counts(n, T, M):
    c = np.empty((n, 2), np.int32)
    c[:, 0], c[:, 1] = T, M
    return c
