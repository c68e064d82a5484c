"""Numpy restatement of the partition of a frame's pixel list among the contexts of a group (include/pt_amd.h
pt_group_partition_host; csrc/pt_group_select.h), and the cases the host and the GPU test share."""
import numpy as np

SHAPES = ((97, 61, 2), (97, 61, 3), (7, 5, 5), (7, 5, 4), (1, 9, 2))  # (W, H, n)
BLOCK = 1024  # list entries a workgroup of the partition's kernels handles


def partition(lst, w, n):
    """([part 0, ..., part n-1], lengths): frame pixel f belongs to context (f // w) % n as tile pixel ((f // w) // n) * w + f % w;
    a part keeps the input order."""
    f = np.asarray(lst, np.int64)
    row = f // w
    owner, tile = row % n, (row // n) * w + f % w
    parts = [tile[owner == i].astype(np.int32) for i in range(n)]
    return parts, np.array([p.size for p in parts], np.int32)


def frame_pixels(part, i, w, n):
    """The inverse, through the stripe formula of a group's tiles: context i's tile starts at frame pixel i * w and holds runs of w
    pixels every n * w; tile pixel p lies at offset p + (p // stripe) * (stride - stripe) from there."""
    p = np.asarray(part, np.int64)
    return i * w + p + (p // w) * (n * w - w)


def cases(w, h, n, seed=5):
    """(name, ascending int32 list) for a frame w x h cut for n contexts."""
    npix = w * h
    rng = np.random.default_rng(seed + 1000 * n + npix)
    every = np.arange(npix, dtype=np.int32)
    rows = np.arange(h)
    out = [("empty", every[:0]), ("first pixel", every[:1]), ("last pixel", every[-1:]), ("every pixel", every)]
    for m in sorted({min(npix, k) for k in (2, 63, 65, npix // 4, BLOCK + 1, 2 * BLOCK, npix - 1)} - {0}):
        out.append((f"random {m}", np.sort(rng.choice(npix, m, replace=False)).astype(np.int32)))
    for i in sorted({0, n - 1}):  # every entry in ONE context's rows: the others get nothing
        mine = every.reshape(h, w)[rows % n == i].reshape(-1)
        out.append((f"only context {i}", mine))
        out.append((f"some of context {i}", mine[rng.random(mine.size) < 0.5]))
    return out
