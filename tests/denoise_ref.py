"""numpy restatement of the edge-avoiding à-trous filter as include/pt_amd.h specifies it (pt_denoise), the reference of
tests/test_denoise_host.py and tests/test_gpu_denoise.py.  Every operand is np.float32, every operation a separate numpy
operation in the stated order; vectorised over the frame, one pass per tap (rows outer, columns inner), a skipped tap adds
weight 0.  Comparisons against it are on bit patterns."""
import numpy as np

f32 = np.float32
H = [f32(1 / 16), f32(1 / 4), f32(3 / 8), f32(1 / 4), f32(1 / 16)]
DEFAULT_SIGMA = (4.0, 0.5, 1.0)
POLY = [f32(1.9875691500e-4), f32(1.3981999507e-3), f32(8.3334519073e-3), f32(4.1665795894e-2), f32(1.6666665459e-1), f32(5.0000001201e-1)]
LOG2E, LN2_HI, LN2_LO = f32(1.44269504), f32(0.693359375), f32(-2.12194440e-4)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def exp32(x):
    """ptmath::exp32 (csrc/pt_portable_math.h) for float32 x <= 0."""
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):  # (arguments far below the cut-off overflow on the way; their result is the +0 below)
        k = np.rint(x * LOG2E)
        r = (x - k * LN2_HI) - k * LN2_LO
        y = np.full_like(x, POLY[0])
        for c in POLY[1:]:
            y = y * r + c
        y = (y * (r * r) + r) + f32(1)
        ki = np.where(x < f32(-80), 0, k).astype(np.int32)
    assert k.dtype == f32 and r.dtype == f32 and y.dtype == f32
    return np.where(x < f32(-80), f32(0), np.ldexp(y, ki)).astype(f32)


def inv_sigma2(sigma, default):
    """1.0f / (sigma * sigma) in float32; 0 in a field = its default, negative = the term off."""
    s = f32(default if sigma == 0 else sigma)
    return f32(0) if s < 0 else f32(1) / (s * s)


def dist2(q, o):
    d = q - o
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def denoise(rgb_sum, planes, w, rows, samples, levels=0, sigma_color=0.0, sigma_normal=0.0, sigma_position=0.0, keep_albedo=False,
            stats=None):
    """rgb_sum [w*rows, 3] SUM image, planes [3, w*rows, 4] feature SUM planes -> averaged radiance [w*rows, 3].
    `stats` (a dict) receives 'cut': taps taken whose exp32 argument was below -80 (weight +0)."""
    levels = levels or 5
    S = np.asarray(rgb_sum, f32).reshape(rows, w, 3)
    s0, s1, s2 = (np.asarray(planes, f32).reshape(3, rows, w, 4)[k] for k in range(3))
    inv_c, inv_n, inv_p = (inv_sigma2(s, d) for s, d in zip((sigma_color, sigma_normal, sigma_position), DEFAULT_SIGMA))
    hit = s1[..., 3] > 0
    den = np.where(hit, s1[..., 3], f32(1))[..., None]
    zero = np.zeros((rows, w, 3), f32)
    n = np.where(hit[..., None], s0[..., :3] / den, zero)
    a = np.where(hit[..., None], s1[..., :3] / den, zero)
    p = np.where(hit[..., None], s2[..., :3] / den, zero)
    c = S / f32(samples)
    demod = (a > 0) & (not keep_albedo)
    c = np.where(demod, c / np.where(demod, a, f32(1)), c)
    ys, xs = np.mgrid[0:rows, 0:w]
    cut = 0
    for l in range(levels):
        s = 1 << l
        cf = inv_c * f32(4 ** l)
        acc = np.zeros((rows, w, 3), f32)
        wsum = np.zeros((rows, w), f32)
        for j in range(-2, 3):
            for i in range(-2, 3):
                y, x = ys + j * s, xs + i * s
                inside = (y >= 0) & (y < rows) & (x >= 0) & (x < w)
                yc, xc = np.clip(y, 0, rows - 1), np.clip(x, 0, w - 1)
                cq = c[yc, xc]
                take = inside & (hit[yc, xc] == hit)
                e = (dist2(cq, c) * cf + dist2(n[yc, xc], n) * inv_n) + dist2(p[yc, xc], p) * inv_p
                wgt = np.where(take, (H[j + 2] * H[i + 2]) * exp32(-e), f32(0))
                cut += int((take & (-e < f32(-80))).sum())
                acc = acc + wgt[..., None] * cq
                wsum = wsum + wgt
        c = acc / wsum[..., None]
        assert c.dtype == f32
    if stats is not None:
        stats["cut"] = cut
    return np.where(demod, c * a, c).reshape(-1, 3)


FRAMES = [(1, 1), (5, 3), (33, 9), (97, 61)]


def random_frame(w, rows, samples=4, seed=0):
    """A frame a renderer would not produce, with everything the filter branches on: hit and miss pixels (misses with stale
    values in their sums), albedo components exactly 0, and colours far enough apart that taps fall below exp32's cut-off.
    Returns (rgb_sum [n, 3], planes [3, n, 4])."""
    rng = np.random.default_rng(1000 * w + rows + seed)
    n = w * rows
    count = rng.integers(0, samples + 1, n).astype(f32)  # iterations that hit; 0 = a miss
    count[rng.random(n) < 0.5] = samples
    if n > 1:
        count[0], count[-1] = 0, samples
    planes = np.zeros((3, n, 4), f32)
    normal = rng.standard_normal((n, 3)).astype(f32)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True).astype(f32)
    albedo = rng.choice(np.array([0.0, 0.2, 0.63, 0.85, 0.98], f32), (n, 3))
    point = (rng.random((n, 3), dtype=f32) * f32(10) - f32(5))
    planes[0, :, :3] = normal * count[:, None]
    planes[0, :, 3] = rng.random(n, dtype=f32) * f32(9) * count
    planes[1, :, :3] = albedo * count[:, None]
    planes[1, :, 3] = count
    planes[2, :, :3] = point * count[:, None]
    planes[2, :, 3] = np.where(count > 0, rng.integers(1, 9, n), 0).astype(np.int32).view(f32)
    stale = (count == 0) & (rng.random(n) < 0.5)  # a miss is decided by the hit count alone
    planes[0, stale, :3] = f32(0.5)
    planes[2, stale, :3] = f32(-3)
    rgb = rng.random((n, 3), dtype=f32) * f32(2) * f32(samples)
    rgb[rng.random(n) < 0.1] *= f32(60)  # fireflies
    rgb[rng.random(n) < 0.05] = 0
    return rgb, planes


def frame_properties(rgb_sum, planes):
    """What the tests assert about an input: (hit pixels, miss pixels, albedo components of hit pixels that are exactly 0)."""
    hit = planes[1, :, 3] > 0
    return int(hit.sum()), int((~hit).sum()), int((planes[1, hit, :3] == 0).sum())
