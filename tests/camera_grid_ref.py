"""Synthetic leaves for the grid build of the camera-dependent tables (pt_stage_camera_grid, pt_camera_grid_host) and a numpy
restatement of that build, independent of both C++ sides.

The frames: root_min = 0, root_max = res as floats, coord_mag = 0.  grid_frame (csrc/pt_tables.cpp) then gives pad = 1e-4 * max(res),
lo = -2 pad and ext = res + 4 pad per axis: a cell is about one unit wide, and a box of half width 0.01 around (cell + 0.5) lies, grown
by the pad, in that one cell (tests/test_camera_grid_host.py asserts it for every tiny leaf of every case).

The restatement: cell_range in float64 with the clamp on the floored double, every leaf's cells leaf by leaf in node order with x
fastest, a stable sort by cell index, `start` as guard zeros + exclusive cumulative counts + the total repeated guard + 1 times, per
record skip = node index and the geom word = neighbour bits 0-5 | (type & 3) << 6 | geom << 8, center_half_box(inner = false) for the
copies.

The node lists interleave inner nodes (geom = -1) with the leaves, so that node index != leaf number; the geom index is a permutation of
the leaf number; the types cycle through 0-2."""
import functools
import math

import numpy as np

NODE = np.dtype([("bmin", np.float32, 3), ("bmax", np.float32, 3), ("skip", np.int32), ("geom", np.int32)])  # capi.TABLE_NODE
BUILT, LIST, CELLS, NONE = 0, 1, 2, 3  # PtCameraGridResult.status
MAX_LIST, MAX_CELLS, MAX_REFS = 4096, 1 << 22, 1 << 22  # ptct::kDeviceMaxList, kDeviceMaxCells, kMaxRefs
PER_BLOCK, PER_PASS = 1024, 256  # cells of a scan workgroup, block sums of a pass of k_ct_scan_sums
FLT_EPSILON = float(np.finfo(np.float32).eps)

# res -> (cells, scan blocks, passes): the issue's table
GRIDS = {
    (1, 1, 1): (1, 1, 1),
    (33, 31, 1): (1023, 1, 1),
    (32, 32, 1): (1024, 1, 1),
    (41, 25, 1): (1025, 2, 1),
    (512, 1, 1): (512, 1, 1),
    (1, 1, 512): (512, 1, 1),
    (3, 5, 7): (105, 1, 1),
    (64, 64, 64): (262144, 256, 1),
    (257, 32, 32): (263168, 257, 2),
    (127, 61, 37): (286639, 280, 2),
    (128, 64, 65): (532480, 520, 3),
    (256, 128, 128): (4194304, 4096, 16),
}
TOO_MANY_CELLS = (257, 128, 128)  # 4,210,688 cells: status CELLS, nothing launched
RANDOM_GRIDS = [(41, 25, 1), (512, 1, 1), (1, 1, 512), (127, 61, 37), (257, 32, 32), (128, 64, 65), (256, 128, 128)]
SLAB_GRIDS = [(64, 64, 64), (127, 61, 37)]
WHOLE = (256, 128, 128)
CROWDED = (257, 32, 32)
CROWDED_CELL = 262144  # the first cell of the second pass


def blocks_and_passes(ncell):
    blocks = (ncell + PER_BLOCK - 1) // PER_BLOCK
    return blocks, (blocks + PER_PASS - 1) // PER_PASS


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def frame(res):
    """pt::grid_frame for root_min = 0, root_max = res, coord_mag = 0: (pad, lo[3], ext[3]) in float64."""
    root_min, root_max = np.zeros(3, np.float32), np.asarray(res, np.float32)
    maxext = float(np.max(root_max.astype(np.float64) - root_min.astype(np.float64)))
    mag = max(0.0, float(np.max(np.abs(root_min))), float(np.max(np.abs(root_max))))
    pad = max(1e-4 * maxext, 64.0 * FLT_EPSILON * mag)
    assert pad < 0.05 * maxext
    lo = root_min.astype(np.float64) - 2.0 * pad
    ext = (root_max.astype(np.float64) + 2.0 * pad) - lo
    return pad, lo, ext


def tiny(res, cells):
    """Boxes of half width 0.01 around the centres of the cells with these indices: [n, 2, 3] float32."""
    c = np.asarray(cells, np.int64)
    xyz = np.stack([c % res[0], (c // res[0]) % res[1], c // (res[0] * res[1])], axis=1).astype(np.float64) + 0.5
    return np.stack([xyz - 0.01, xyz + 0.01], axis=1).astype(np.float32)


def per_block_cells(res):
    ncell = res[0] * res[1] * res[2]
    blocks, _ = blocks_and_passes(ncell)
    cells = [b * PER_BLOCK for b in range(blocks) for _ in range(1 + b % 3)]
    return np.asarray(cells + [ncell - 1], np.int64)


def node_list(boxes, inner_before, root_max):
    """Leaves with these boxes, leaf j behind an inner node where inner_before[j]; (nodes, geom_types, leaf node indices)."""
    L = boxes.shape[0]
    inner_before = np.asarray(inner_before, bool)
    index = np.arange(L) + np.cumsum(inner_before)  # node index of leaf j
    nodes = np.zeros(L + int(inner_before.sum()), NODE)
    nodes["bmax"] = np.asarray(root_max, np.float32)  # inner nodes: the root's box
    nodes["geom"] = -1
    nodes["skip"] = np.arange(nodes.size) + 1
    step = L // 2 + 1
    while math.gcd(step, L) != 1:
        step += 1
    geom = (np.arange(L, dtype=np.int64) * step + L // 3) % L  # a permutation of the leaf numbers
    nodes["bmin"][index], nodes["bmax"][index], nodes["geom"][index] = boxes[:, 0], boxes[:, 1], geom
    return nodes, (np.arange(L) % 3).astype(np.int32), index


def regular(boxes, res):
    return node_list(boxes, np.arange(boxes.shape[0]) % 3 != 1, res)


def random_boxes(res, n=20000, seed=20240):
    """Extents of 0 to 3 cells per axis; a third with the lower face (grown by the pad) on a cell boundary, a third with the upper one;
    one in eight pushed partly or wholly outside the frame."""
    rng = np.random.default_rng(seed + res[0] * 7 + res[1] * 3 + res[2])
    pad, lo, ext = frame(res)
    r = np.asarray(res, np.float64)
    w = ext / r
    size = rng.uniform(0.0, 3.0, (n, 3)) * (rng.random((n, 3)) > 0.1)  # (one axis in ten flat)
    a = rng.uniform(0.0, 1.0, (n, 3)) * r - 0.5 * size
    kind = rng.integers(0, 3, n)
    k = rng.integers(0, np.asarray(res) + 1, (n, 3)).astype(np.float64)
    a = np.where((kind == 1)[:, None], lo + k * w + pad, a)           # bmin - pad on the boundary
    a = np.where((kind == 2)[:, None], lo + k * w - pad - size, a)    # bmax + pad on the boundary
    out = rng.integers(0, 8, n) == 0
    a = a + np.where(out[:, None], rng.choice([-1.0, 1.0], (n, 3)) * rng.uniform(0.0, 1.2, (n, 3)) * r, 0.0)
    bmin = a.astype(np.float32)
    bmax = np.maximum((a + size).astype(np.float32), bmin)
    return np.stack([bmin, bmax], axis=1)


def slab_boxes(res):
    r = np.asarray(res, np.float32)
    z, x, y = res[2] // 2 + 0.5, res[0] // 3 + 0.5, res[1] // 4 + 0.5
    wall = [[0.0, 0.0, z - 0.01], [r[0], r[1], z + 0.01]]      # one whole z-layer
    column = [[x - 0.01, y - 0.01, 0.0], [x + 0.01, y + 0.01, r[2]]]  # along z: stride nx * ny between its cells
    whole = [[0.0, 0.0, 0.0], list(r)]
    return np.concatenate([np.asarray([wall, column, whole], np.float32), tiny(res, per_block_cells(res))])


def whole_boxes(res, n, extra_tiny=0):
    b = np.zeros((n, 2, 3), np.float32)
    b[:, 1] = np.asarray(res, np.float32)
    return np.concatenate([b, tiny(res, [5] * extra_tiny)]) if extra_tiny else b


def crowded(res, cell, n, seed=77):
    """n tiny leaves in one cell, each box a little different, behind irregular runs of inner nodes."""
    rng = np.random.default_rng(seed)
    b = tiny(res, [cell] * n).astype(np.float64)
    b += (rng.permutation(n)[:, None, None] / n - 0.5) * 0.008  # (moved as a whole: by less than 0.004)
    return node_list(b.astype(np.float32), rng.random(n) < 0.4, res)


@functools.lru_cache(maxsize=None)
def case_names():
    names = [("per_block", g) for g in GRIDS] + [("per_block", TOO_MANY_CELLS)]
    names += [("random", g) for g in RANDOM_GRIDS] + [("slabs", g) for g in SLAB_GRIDS]
    names += [("whole_1", WHOLE), ("whole_1_and_tiny", WHOLE), ("whole_1100", WHOLE), ("crowded_4096", CROWDED), ("crowded_4097", (3, 5, 7))]
    return names


def center_halves(name):
    """The center_half values a case runs with: both, except whole_grid (and the cases that build nothing either way)."""
    return (0,) if name[0].startswith("whole") else (0, 1)


def case(name):
    """(nodes, geom_types, leaf node indices, tiny-leaf mask or None) of a case; root_min = 0 and root_max = res."""
    kind, res = name
    if kind == "per_block":
        return regular(tiny(res, per_block_cells(res)), res)
    if kind == "random":
        return regular(random_boxes(res), res)
    if kind == "slabs":
        return regular(slab_boxes(res), res)
    if kind == "whole_1":
        return regular(whole_boxes(res, 1), res)
    if kind == "whole_1_and_tiny":
        return regular(whole_boxes(res, 1, 1), res)
    if kind == "whole_1100":
        return regular(whole_boxes(res, 1100), res)
    if kind == "crowded_4096":
        return crowded(res, CROWDED_CELL, 4096)
    if kind == "crowded_4097":
        return crowded(res, 52, 4097)
    raise KeyError(name)


def case_id(name):
    return "%s-%dx%dx%d" % ((name[0],) + tuple(name[1]))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def cell_range(bmin, bmax, res):
    """ptct::cell_range over arrays of boxes, float64: (c0, c1) as [n, 3] int64."""
    pad, lo, ext = frame(res)
    r = np.asarray(res, np.float64)

    def clamp(v):  # on the floored double, before the conversion; a NaN: cell 0
        return np.clip(np.where(np.isnan(v), 0.0, v), 0.0, r - 1.0).astype(np.int64)

    c0 = clamp(np.floor(((bmin.astype(np.float64) - pad) - lo) / ext * r))
    c1 = clamp(np.floor(((bmax.astype(np.float64) + pad) - lo) / ext * r))
    return c0, c1


def center_half(bmin, bmax):
    """ptct::center_half_box(inner = false): centre rounded to float, half extent rounded up from the farther face."""
    lo, hi = bmin.astype(np.float64), bmax.astype(np.float64)
    c = (0.5 * (lo + hi)).astype(np.float32)
    a, b = hi - c.astype(np.float64), c.astype(np.float64) - lo
    h = np.where(a < b, b, a)
    hf = h.astype(np.float32)
    up = np.nextafter(hf, np.float32(np.inf))
    return c, np.where(hf.astype(np.float64) < h, up, hf).astype(np.float32)


def shape_words(res):
    """pt::grid_shape: origin, cell_size, inv_cell_size (float32 [3] each) and pad (float32)."""
    pad, lo, ext = frame(res)
    r = np.asarray(res, np.float64)
    return lo.astype(np.float32), (ext / r).astype(np.float32), (r / ext).astype(np.float32), np.float32(pad)


def restate(nodes, geom_types, res, with_copies):
    """dict(status, ncell, guard, refs, longest) and, when built, start, items [refs, 8] uint32 and items_b (or None)."""
    ncell = res[0] * res[1] * res[2]
    guard = res[0] * res[1] + res[0] + 2
    out = dict(status=BUILT, ncell=ncell, guard=guard, refs=0, longest=0, start=None, items=None, items_b=None)
    if ncell > MAX_CELLS:
        out["status"] = CELLS
        return out
    leaf = np.flatnonzero(nodes["geom"] >= 0)
    c0, c1 = cell_range(nodes["bmin"][leaf], nodes["bmax"][leaf], res)
    n = c1 - c0 + 1
    per_leaf = n[:, 0] * n[:, 1] * n[:, 2]
    refs = out["refs"] = int(per_leaf.sum())
    if refs > MAX_REFS or refs == 0:
        out["status"] = NONE
        return out
    owner = np.repeat(np.arange(leaf.size), per_leaf)  # leaf by leaf in node order
    k = np.arange(refs) - np.repeat(np.cumsum(per_leaf) - per_leaf, per_leaf)
    nx, nxy = n[owner, 0], n[owner, 0] * n[owner, 1]
    z = k // nxy
    y = (k - z * nxy) // nx
    x = k - z * nxy - y * nx  # x fastest
    x, y, z = x + c0[owner, 0], y + c0[owner, 1], z + c0[owner, 2]
    cell = x + res[0] * (y + res[1] * z)
    counts = np.bincount(cell, minlength=ncell)
    out["longest"] = int(counts.max())
    if out["longest"] > MAX_LIST:
        out["status"] = LIST
        return out
    order = np.argsort(cell, kind="stable")
    owner, x, y, z = owner[order], x[order], y[order], z[order]
    ends = np.cumsum(counts)
    out["start"] = np.concatenate([np.zeros(guard, np.int64), ends - counts, np.full(guard + 1, refs, np.int64)]).astype(np.uint32)
    node = leaf[owner]
    geom = nodes["geom"][node].astype(np.int64)
    word = ((x > c0[owner, 0]) * 1 | (x < c1[owner, 0]) * 2 | (y > c0[owner, 1]) * 4 | (y < c1[owner, 1]) * 8 | (z > c0[owner, 2]) * 16 |
            (z < c1[owner, 2]) * 32 | (np.asarray(geom_types, np.int64)[geom] & 3) << 6 | geom << 8)
    items = np.zeros((refs, 8), np.uint32)
    items[:, 0:3] = nodes["bmin"][node].view(np.uint32)
    items[:, 3:6] = nodes["bmax"][node].view(np.uint32)
    items[:, 6] = node.astype(np.uint32)
    items[:, 7] = word.astype(np.uint32)
    out["items"] = items
    if with_copies:
        c, h = center_half(nodes["bmin"][node], nodes["bmax"][node])
        out["items_b"] = items.copy()
        out["items_b"][:, 0:3], out["items_b"][:, 3:6] = c.view(np.uint32), h.view(np.uint32)
    return out


def first_difference(a, b, guard, what):
    """Where two cell tables differ: the first cells with their scan block and pass, for a failure message (None when equal)."""
    if a.shape != b.shape:
        return "%s: %d words against %d" % (what, a.size, b.size)
    bad = np.flatnonzero(a != b)
    if bad.size == 0:
        return None
    lines = ["%s: %d of %d words differ" % (what, bad.size, a.size)]
    for i in bad[:8]:
        c = int(i) - guard
        lines.append("  word %d (cell %d, block %d, pass %d): %d against %d" % (i, c, c // PER_BLOCK, c // PER_BLOCK // PER_PASS, a[i], b[i]))
    return "\n".join(lines)


def first_record_difference(a, b, start, guard, what):
    """Where two record arrays differ: the first records, the cell each lies in, its block and pass (None when equal)."""
    if a.shape != b.shape:
        return "%s: %d records against %d" % (what, a.shape[0], b.shape[0])
    bad = np.flatnonzero((a != b).any(axis=1))
    if bad.size == 0:
        return None
    cells = start[guard:-guard - 1].astype(np.int64)
    lines = ["%s: %d of %d records differ" % (what, bad.size, a.shape[0])]
    for i in bad[:8]:
        c = int(np.searchsorted(cells, i, side="right")) - 1
        lines.append("  record %d (cell %d, block %d, pass %d): %s against %s" % (i, c, c // PER_BLOCK, c // PER_BLOCK // PER_PASS, a[i], b[i]))
    return "\n".join(lines)
