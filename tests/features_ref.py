"""Reference of the first-hit feature buffers (include/pt_amd.h: pt_render_features) for tests/test_gpu_features*.py:
the oracle's generate + intersect in PORTABLE mode, per iteration, accumulated in float32 in iteration order.  Every
per-iteration record is computed once per (scene, resolution, jitter, iteration), shared and read-only."""
import numpy as np

KEYS = ("normal", "depth", "albedo", "hits", "position", "object_id")
_PER_ITERATION = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def iteration_values(ob, path, res, aa, it):
    """What iteration `it` adds for every pixel of the frame (zeros where the camera ray misses) + the geom types."""
    key = (path, tuple(res), bool(aa), it if aa else 0)  # without jitter every iteration has the same ray
    if key not in _PER_ITERATION:
        ob.set_math_mode(ob.PORTABLE)
        ob.load_scene(path, res=res)
        try:
            ob.set_aa_jitter(bool(aa))
            o, d = ob.generate(0, res[0] * res[1], iteration=it)
            h = ob.intersect(o, d)
        finally:
            ob.set_aa_jitter(False)
        colors = np.array([[m.color[0], m.color[1], m.color[2]] for m in ob.materials()], np.float32)
        hit = h["t"] >= 0
        zero3 = np.zeros((hit.size, 3), np.float32)
        v = dict(normal=np.where(hit[:, None], h["nrm"].T, zero3), depth=np.where(hit, h["t"], np.float32(0)),
                 albedo=np.where(hit[:, None], colors[np.where(hit, h["mat"], 0)], zero3), hits=hit.astype(np.float32),
                 position=np.where(hit[:, None], h["pt"].T, zero3), object_id=np.where(hit, h["geom"] + 1, 0).astype(np.int32),
                 geom_types=np.array([g.type for g in ob.geoms()], np.int32))
        for a in v.values():
            a.setflags(write=False)
        _PER_ITERATION[key] = v
    return _PER_ITERATION[key]


def reference(ob, path, res, aa, first, last, sel=slice(None)):
    """The SUM buffers after iterations first .. last for the frame pixels `sel` (tile order)."""
    acc = None
    for it in range(first, last + 1):
        v = iteration_values(ob, path, res, aa, it)
        if acc is None:
            acc = {k: np.zeros_like(v[k][sel]) for k in KEYS}
        for k in KEYS[:-1]:
            acc[k] = acc[k] + v[k][sel]  # float32, iteration order
        acc["object_id"] = v["object_id"][sel]
    return acc


def stripe_rows(res, pixel_begin, pixel_count, stripe_stride):
    """Frame pixel indices of a tile of whole rows, every (stripe_stride / width)-th row from pixel_begin."""
    w = res[0]
    rows = np.arange(pixel_begin // w, res[1], stripe_stride // w)[:pixel_count // w]
    return (rows[:, None] * w + np.arange(w)[None, :]).reshape(-1)


def assert_same(got, want, what=""):
    for k in KEYS:
        a, b = bits(got[k]), bits(want[k])
        assert a.shape == b.shape, f"{what} {k}: {a.shape} vs {b.shape}"
        bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
        assert bad.size == 0, f"{what} {k}: {bad.size} of {a.shape[0]} pixels differ, first {bad[:8]}"
