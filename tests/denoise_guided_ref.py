"""numpy restatement of the variance-guided form of the à-trous filter as include/pt_amd.h specifies it (pt_denoise_guided), the
reference of tests/test_denoise_guided_host.py and tests/test_gpu_denoise_guided.py.  Like denoise_ref, whose exp32, dist2, H and
bits it uses: every operand np.float32, every operation a separate numpy operation in the stated order, vectorised over the
frame, one pass per tap (rows outer, columns inner), a skipped tap adds +0.  Comparisons against it are on bit patterns."""
import numpy as np

import noise_ref
from denoise_ref import H, bits, dist2, exp32, inv_sigma2  # noqa: F401  (bits: for the tests)

f32 = np.float32
G = [f32(1 / 4), f32(1 / 2), f32(1 / 4)]
FLOOR = f32(1e-8)  # PT_DENOISE_VARIANCE_FLOOR
DEFAULT_SIGMA = (8.0, 0.5, 1.0)


def denoise_guided(rgb_sum, planes, noise, w, rows, groups, iters, levels=0, sigma_color=0.0, sigma_normal=0.0, sigma_position=0.0,
                   keep_albedo=False, stats=None):
    """rgb_sum [w*rows, 3] SUM image, planes [3, w*rows, 4] feature SUM planes, noise [2, w*rows, 4] the fold's planes after
    `groups` folds of `iters` iterations in all -> averaged radiance [w*rows, 3].  `stats` (a dict) receives var_raw, var_0 and
    var (the variance after the last level), [w*rows] each, and 'cut' as in denoise_ref."""
    levels = levels or 5
    S = np.asarray(rgb_sum, f32).reshape(rows, w, 3)
    s0, s1, s2 = (np.asarray(planes, f32).reshape(3, rows, w, 4)[k] for k in range(3))
    prev, q = (np.asarray(noise, f32).reshape(2, rows, w, 4)[k][..., :3] for k in range(2))
    inv_c, inv_n, inv_p = (inv_sigma2(s, d) for s, d in zip((sigma_color, sigma_normal, sigma_position), DEFAULT_SIGMA))
    Tf = f32(iters)
    Df = f32(groups - 1) * Tf
    assert groups >= 2 and Df.dtype == f32
    # prepare
    hit = s1[..., 3] > 0
    den = np.where(hit, s1[..., 3], f32(1))[..., None]
    zero = np.zeros((rows, w, 3), f32)
    n = np.where(hit[..., None], s0[..., :3] / den, zero)
    a = np.where(hit[..., None], s1[..., :3] / den, zero)
    p = np.where(hit[..., None], s2[..., :3] / den, zero)
    c = S / Tf
    demod = (a > 0) & (not keep_albedo)
    safe_a = np.where(demod, a, f32(1))
    c = np.where(demod, c / safe_a, c)
    with np.errstate(under="ignore"):
        d = q - (prev * prev) / Tf
        v = np.where(d > 0, d, f32(0)) / Df
        v = np.where(demod, v / (safe_a * safe_a), v)
    var_raw = (v[..., 0] + v[..., 1]) + v[..., 2]
    assert c.dtype == f32 and var_raw.dtype == f32
    ys, xs = np.mgrid[0:rows, 0:w]

    def tap(dy, dx):
        y, x = ys + dy, xs + dx
        inside = (y >= 0) & (y < rows) & (x >= 0) & (x < w)
        yc, xc = np.clip(y, 0, rows - 1), np.clip(x, 0, w - 1)
        return yc, xc, inside & (hit[yc, xc] == hit)

    # variance prefilter
    acc, gsum = np.zeros((rows, w), f32), np.zeros((rows, w), f32)
    with np.errstate(under="ignore"):
        for j in range(-1, 2):
            for i in range(-1, 2):
                yc, xc, take = tap(j, i)
                g = G[j + 1] * G[i + 1]
                acc = acc + np.where(take, g * var_raw[yc, xc], f32(0))
                gsum = gsum + np.where(take, g, f32(0))
        var = acc / gsum
    var_0 = var
    cut = 0
    for l in range(levels):
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


def group_sizes(groups, iters):
    """`iters` iterations in `groups` groups: equal sizes, the remainder in the last."""
    sizes = [iters // groups] * groups
    sizes[-1] += iters - sum(sizes)
    assert min(sizes) >= 1
    return sizes


def random_noise_planes(w, rows, groups, iters, seed=0):
    """The planes [2, w*rows, 4] noise_ref's fold leaves after `groups` folds over noise_ref.random_sums' made-up render of `iters`
    iterations: prev (= the SUM image the filter is given, planes[0, :, :3]) | w and q | 0.  The pixel classes of random_sums give
    all-zero and constant pixels (variance 0, or a rounding residue d on either side of 0) and pixels around 1e-20 and 1e-30 next
    to ordinary ones (variances many decades apart, denormal ones among them)."""
    npix = w * rows
    sizes = group_sizes(groups, iters)
    sums, _ = noise_ref.random_sums(npix, sizes, 7000 * w + 13 * rows + seed)
    planes, T = noise_ref.new_planes(npix), 0
    for M, (n, S) in enumerate(zip(sizes, sums), start=1):
        T += n
        noise_ref.fold(S, planes, n, M, T)
    return planes


def noise_properties(planes, groups, iters):
    """What the tests assert about the planes: (components with d <= 0, pixels of variance 0, decades between the smallest
    positive and the largest variance)."""
    prev, q, var = planes[0, :, :3], planes[1, :, :3], planes[0, :, 3]
    with np.errstate(under="ignore"):
        d = q - (prev * prev) / f32(iters)
    pos = var[var > 0].astype(np.float64)
    decades = float(np.log10(pos.max() / pos.min())) if pos.size else 0.0
    return int((d <= 0).sum()), int((var == 0).sum()), decades
