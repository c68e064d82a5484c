"""numpy restatement of adaptive sampling's key, selection, merge and resolve (include/pt_amd.h pt_adaptive_round;
csrc/pt_adaptive.h), float32 operation by operation in the stated order, like noise_ref.py for the fold.  numpy's float32 +, *, /
are the IEEE operations and keep denormals, so pt_adaptive_select_host / pt_adaptive_merge_host and the device's kernels must equal
this bit for bit.  Also the shapes, list lengths and estimate patterns the host and the GPU tests share."""
import math

import numpy as np

import noise_ref
from noise_ref import bits, f32  # noqa: F401

SHAPES = ((1, 1), (5, 1), (1, 7), (64, 1), (97, 11), (97, 61))  # W x R; 97 x 11 = 1067 pixels, just past one block of 1024
PATTERNS = ("random", "zero", "equal", "three", "low10", "mid11", "mixedT")
G = (f32(0.25), f32(0.5), f32(0.25))


def list_lengths(n):
    """m in {1, 2, ceil(n / 4), n - 1, n}, those that exist."""
    return sorted({m for m in (1, 2, -(-n // 4), n - 1, n) if 1 <= m <= n})


def list_length(fraction, n):
    return int(min(n, max(1, math.ceil(float(fraction) * n))))


def keys(w, W, R, counts):
    """The uint32 sort keys [W * R] from the estimates w [W * R] float32 and the counts [W * R, 2] int32."""
    w = np.ascontiguousarray(w, f32).reshape(R, W)
    Tf = counts[:, 0].astype(f32).reshape(R, W)
    with np.errstate(all="ignore"):
        s = (w * Tf).astype(f32)
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
        key = ((num / den).astype(f32) / Tf).astype(f32)
    out = bits(key).reshape(-1).copy()
    out[np.isnan(key).reshape(-1)] = 0xFFFFFFFF  # a NaN sorts first, whatever its sign and payload
    return out


def select(w, W, R, counts, m):
    """The m tile indices with the largest key, equal keys by the smaller index, ascending (int32 [m])."""
    k = keys(w, W, R, counts)
    order = np.lexsort((np.arange(k.size), -k.astype(np.int64)))  # key descending, then index ascending
    return np.sort(order[:m]).astype(np.int32)


def merge(S, planes, counts, lst, Sw, G_iters):
    """One merge, in place: S [n, 3] float32, planes [2, n, 4] float32, counts [n, 2] int32; lst [m] and Sw [m, 3] the list and its
    group sums of G_iters iterations.  Returns SSE_est = float64 sum of w over ALL pixels in pixel order."""
    lst = np.asarray(lst, np.int64)
    Sw = np.ascontiguousarray(Sw, f32)
    nf = f32(G_iters)
    with np.errstate(all="ignore"):
        Sp = (S[lst] + Sw).astype(f32)
        q = (planes[1, lst, :3] + ((Sw * Sw).astype(f32) / nf).astype(f32)).astype(f32)
        T = counts[lst, 0] + np.int32(G_iters)
        M = counts[lst, 1] + np.int32(1)
        Tf = T.astype(f32)
        Df = ((M - 1).astype(f32) * Tf).astype(f32)
        d = (q - ((Sp * Sp).astype(f32) / Tf[:, None]).astype(f32)).astype(f32)
        v = (np.where(d > 0, d, f32(0)).astype(f32) / Df[:, None]).astype(f32)
        w = ((v[:, 0] + v[:, 1]).astype(f32) + v[:, 2]).astype(f32)
    S[lst] = Sp
    planes[0, lst, :3], planes[0, lst, 3] = Sp, w
    planes[1, lst, :3], planes[1, lst, 3] = q, f32(0)
    counts[lst, 0], counts[lst, 1] = T, M
    return float(np.cumsum(planes[0, :, 3].astype(np.float64))[-1])  # (cumsum adds in index order; add.reduce adds pairwise)


def resolve(S, counts):
    with np.errstate(all="ignore"):
        return (np.ascontiguousarray(S, f32) / counts[:, 0].astype(f32)[:, None]).astype(f32)


def uniform_counts(n, T, M):
    c = np.empty((n, 2), np.int32)
    c[:, 0], c[:, 1] = T, M
    return c


def pattern(name, W, R, seed=0):
    """(noise planes [2, n, 4] float32, counts [n, 2] int32) of a made-up tile whose estimates w exercise one property of the
    selection.  With `equal` T everywhere and a constant w the prefiltered key is w again only up to rounding of the border
    normalisation, so the tie patterns are built on exact binary fractions: G-weighted sums of equal values then stay exact."""
    n = W * R
    rng = np.random.default_rng(1000 * seed + 31 * W + R)
    planes = noise_ref.new_planes(n)
    planes[0, :, :3] = rng.uniform(0, 4, (n, 3)).astype(f32)  # the selection must not look at these
    planes[1, :, :3] = rng.uniform(0, 9, (n, 3)).astype(f32)
    counts = uniform_counts(n, 8, 2)
    if name == "random":
        w = (rng.exponential(1.0, n) ** 3 * 1e-3).astype(f32)
        w[rng.random(n) < 0.4] = 0  # the zero-variance half of a frame
    elif name == "zero":
        w = np.zeros(n, f32)
    elif name == "equal":
        w = np.full(n, 0.375, f32)
    elif name == "three":  # three distinct values in column bands: inside a band the keys are exactly equal in every row, so the ties
        w = np.array([0.25, 0.5, 1.0], f32)[((np.arange(n) % W) // 5 + (np.arange(n) // W) // 23) % 3]  # at tau straddle waves and blocks
    elif name == "low10":  # keys that differ only in their low 10 bits: the last radix pass decides
        w = (np.uint32(0x3E800000) + rng.integers(0, 1 << 10, n).astype(np.uint32)).view(f32)
    elif name == "mid11":  # keys that differ only in bits 10..20: the middle pass decides
        w = (np.uint32(0x3E800000) + (rng.integers(0, 1 << 11, n).astype(np.uint32) << np.uint32(10))).view(f32)
    elif name == "mixedT":  # pixels with different iteration counts, as after some rounds
        w = (rng.exponential(1.0, n) * 1e-2).astype(f32)
        counts[:, 0] = 8 + 4 * rng.integers(0, 6, n)
        counts[:, 1] = 2 + (counts[:, 0] - 8) // 4
    else:
        raise KeyError(name)
    planes[0, :, 3] = w
    return planes, counts

