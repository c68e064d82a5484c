"""numpy restatement of the noise estimate's fold (include/pt_amd.h pt_noise_fold; csrc/pt_noise.h), float32 operation by
operation in the stated order.  numpy's float32 +, -, *, / are the IEEE operations and keep denormals, so the planes of
pt_noise_fold_host and of the device's k_noise_fold must equal this bit for bit."""
import numpy as np

f32 = np.float32
PLANES = 2
PIXELS = (1, 63, 64, 65, 1025, 2049)  # one pixel, around a wave, past one and two workgroups' 1024
SEQUENCES = ((1, 3, 25, 7, 16), (16, 1), (7, 7, 7), (25,), (3, 1, 16, 25, 7, 1))  # group sizes n, all from {1, 3, 25, 7, 16}


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def new_planes(n):
    return np.zeros((PLANES, n, 4), f32)


def fold(S, planes, n, M, T):
    """One fold: S [npix, 3] float32 SUM image; planes [2, npix, 4] updated in place; n the group's iterations, M and T the
    groups and iterations AFTER it.  Returns (w [npix] float32, SSE_est = float64 sum of w in pixel order, or -1 when M < 2)."""
    S = np.ascontiguousarray(S, f32)
    nf, Tf = f32(n), f32(T)
    Df = f32(f32(M - 1) * Tf)
    prev, q = planes[0, :, :3], planes[1, :, :3]
    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        b = (S - prev).astype(f32)
        bb = (b * b).astype(f32)
        q[:] = (q + (bb / nf).astype(f32)).astype(f32)
        prev[:] = S
        if M >= 2:
            ss = (S * S).astype(f32)
            d = (q - (ss / Tf).astype(f32)).astype(f32)
            v = (np.where(d > 0, d, f32(0)).astype(f32) / Df).astype(f32)
            w = ((v[:, 0] + v[:, 1]).astype(f32) + v[:, 2]).astype(f32)
        else:
            w = np.zeros(S.shape[0], f32)
    planes[0, :, 3] = w
    planes[1, :, 3] = f32(0)
    sse = float(np.add.reduce(w.astype(np.float64))) if M >= 2 else -1.0
    return w, sse


def random_sums(npix, groups, seed):
    """Running SUM images after each group of a made-up render: [len(groups)] arrays [npix, 3].  Per-sample radiance is
    mean + spread * noise with pixel classes the fold branches on: ordinary pixels, all-zero pixels, constant pixels (every
    group sum is exactly n * c, so d = q - S^2 / T is a rounding residue on either side of 0), pixels around 1e-30 (b * b
    underflows to zero) and around 1e-20 (b * b and (b * b) / n are denormal)."""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 5, npix) if npix > 4 else np.arange(npix) % 5
    mean = rng.uniform(0.0, 2.0, (npix, 3))
    const = rng.choice(np.array([0.1, 0.3, 1.0 / 3.0, 0.7, 1.7, 2.5e-3]), (npix, 3))
    scale = np.where(cls == 3, 1e-30, np.where(cls == 4, 1e-20, 1.0))[:, None]
    S = np.zeros((npix, 3), f32)
    out = []
    for n in groups:
        for _ in range(n):  # sample by sample, as the renderer accumulates
            x = mean * rng.exponential(1.0, (npix, 3)) * scale
            x = np.where((cls == 2)[:, None], const, x)
            x = np.where((cls == 1)[:, None], 0.0, x)
            S = (S + x.astype(f32)).astype(f32)
        out.append(S.copy())
    return out, cls
