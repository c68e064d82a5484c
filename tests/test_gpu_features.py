"""First-hit feature buffers (pt_render_features, csrc/pt_features.inc): per pixel the running sums of normal, hit
distance, material colour, hit count and intersection point of the camera ray of every iteration, and the object id of
the last one.  Depth 0 runs the reference's arithmetic in every build, so everything here is compared on bit patterns
against the oracle's generate + intersect (PORTABLE mode) accumulated in float32 in iteration order — no tolerance."""
import numpy as np
import pytest

from features_ref import KEYS, assert_same, bits, iteration_values, reference, stripe_rows

pytestmark = pytest.mark.gpu
RES = (97, 61)  # 5917 pixels = 92 groups of 64 + 29: the tail group is masked
TILE = dict(pixel_begin=97 * 7, pixel_count=97 * 20, stripe_pixels=97, stripe_stride=194)
_GPU = {}


def features(path, res, calls, **kw):
    """The feature buffers after render_features(first, count) for every (first, count) of `calls` (cached per argument set)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    key = (path, tuple(res), tuple(calls), tuple(sorted(kw.items())))
    if key not in _GPU:
        r = capi.Renderer(capi.Scene(path, res=res), **kw)
        try:
            for first, count in calls:
                r.render_features(first, count)
            _GPU[key] = r.readback_features()
        finally:
            r.free()
    return _GPU[key]


def test_whole_frame_accumulates_across_calls(scene_dir, oracle):
    path = scene_dir["cornell"]
    got = features(path, RES, ((1, 1), (2, 3)))
    want = reference(oracle, path, RES, False, 1, 4)
    frac = (want["hits"] > 0).mean()
    assert 0.2 < frac < 0.8, frac  # the input has hits and misses
    assert_same(got, want, "iterations 1..4")
    assert np.array_equal(got["hits"][want["hits"] > 0], np.full(int((want["hits"] > 0).sum()), 4, np.float32))


def test_repeated_adds_are_not_a_multiply(scene_dir, oracle):
    """Without jitter the ray is traced once per call, but its values are ADDED once per iteration: from six adds on the
    float32 running sum differs from count * value in the last bit for thousands of components of this frame (up to five
    adds it does not, so the four iterations above cannot tell)."""
    path = scene_dir["cornell"]
    want = reference(oracle, path, RES, False, 1, 7)
    v = iteration_values(oracle, path, RES, False, 1)
    assert sum(int((bits(want[k]) != bits(np.float32(7) * v[k])).sum()) for k in ("normal", "depth", "position")) >= 1000
    assert_same(features(path, RES, ((1, 3), (4, 4))), want, "iterations 1..7")


# rows 7, 9, .., 45 of the frame: the tile of tests/test_aa_extension.py.  This frame has 174 pixels with fractional coverage after
# five jittered iterations, 90 of them in rows 3 and 58 (the box's top and bottom edges), which that tile does not own: it holds
# 35.  SECOND_TILE is the same shape two row pairs higher (rows 3, 5, .., 41) and holds more than 50.
SECOND_TILE = dict(TILE, pixel_begin=97 * 3)


def striped_case(scene_dir, oracle, arith, tile=TILE, min_partial=35):
    path = scene_dir["cornell"]
    kw = dict(aa_jitter=True, iters_per_batch=3, arith=arith, **tile)
    sel = stripe_rows(RES, tile["pixel_begin"], tile["pixel_count"], tile["stripe_stride"])
    whole = reference(oracle, path, RES, True, 1, 5)
    assert int(((whole["hits"] > 0) & (whole["hits"] < 5)).sum()) >= 174
    want = reference(oracle, path, RES, True, 1, 5, sel)
    partial = int(((want["hits"] > 0) & (want["hits"] < 5)).sum())
    assert partial >= min_partial, partial  # edges with fractional coverage: a genuine accumulation (a condition on the input)
    one = features(path, RES, ((1, 5),), **kw)
    two = features(path, RES, ((1, 2), (3, 3)), **kw)
    assert_same(one, want, f"{arith}: one call")
    assert_same(two, want, f"{arith}: two calls")
    assert np.array_equal(one["object_id"], iteration_values(oracle, path, RES, True, 5)["object_id"][sel])
    return one


def test_striped_tile_with_jitter(scene_dir, oracle):
    striped_case(scene_dir, oracle, "exact")


def test_striped_tile_with_fifty_partially_covered_pixels(scene_dir, oracle):
    striped_case(scene_dir, oracle, "exact", SECOND_TILE, 50)


@pytest.mark.parametrize("arith", ["fma", "fast"])
def test_modes_are_bit_identical(scene_dir, oracle, arith):
    for tile, min_partial in ((TILE, 35), (SECOND_TILE, 50)):
        got = striped_case(scene_dir, oracle, arith, tile, min_partial)
        exact = features(scene_dir["cornell"], RES, ((1, 5),), aa_jitter=True, iters_per_batch=3, arith="exact", **tile)
        assert_same(got, exact, f"{arith} vs exact")


@pytest.mark.parametrize("begin", [100, 97 * 30 + 60])  # beside the box (all misses) / across its right edge and a row end
def test_tile_smaller_than_a_group(scene_dir, oracle, begin):
    path = scene_dir["cornell"]
    got = features(path, RES, ((1, 3),), aa_jitter=True, pixel_begin=begin, pixel_count=37)
    assert got["hits"].shape == (37,)
    want = reference(oracle, path, RES, True, 1, 3, slice(begin, begin + 37))
    assert (want["hits"] > 0).any() == (begin != 100) and (want["hits"] == 0).any()
    assert_same(got, want, "37 pixels")


@pytest.mark.parametrize("lds_table_kb", [64, -1])
def test_table_placement(scene_dir, oracle, lds_table_kb):
    path = scene_dir["cornell"]
    got = features(path, RES, ((1, 1),), lds_table_kb=lds_table_kb)
    assert_same(got, reference(oracle, path, RES, False, 1, 1), f"lds_table_kb={lds_table_kb}")
    assert_same(got, features(path, RES, ((1, 1),)), "default placement")


@pytest.mark.parametrize("debug_flags", [0, 256])
def test_large_scene_packet_scan(scene_dir, oracle, debug_flags):
    path, res = scene_dir["stress_big"], (160, 90)
    first = iteration_values(oracle, path, res, True, 1)
    assert np.unique(first["object_id"][first["object_id"] > 0]).size >= 100
    got = features(path, res, ((1, 3),), aa_jitter=True, debug_flags=debug_flags)
    assert_same(got, reference(oracle, path, res, True, 1, 3), f"debug_flags={debug_flags}")


def test_triangle_mesh(oracle, tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    res = (200, 120)
    path = scenes.write_scene(scenes.mesh_scene_text(), str(tmp_path / "mesh.txt"))
    want = reference(oracle, path, res, False, 1, 2)
    types = iteration_values(oracle, path, res, False, 1)["geom_types"]
    got = features(path, res, ((1, 2),))
    assert_same(got, want, "mesh")
    ids = got["object_id"][got["object_id"] > 0]
    assert (types[ids - 1] == 2).any()  # PT_GEOM_TRIANGLE


def test_independent_of_the_image(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path = scene_dir["cornell"]
    kw = dict(aa_jitter=True, iters_per_batch=3)
    n = RES[0] * RES[1]
    r = capi.Renderer(capi.Scene(path, res=RES), **kw)
    try:
        r.render(1, 4)
        before = r.stats().device_bytes
        r.render_features(1, 4)
        assert r.stats().device_bytes == before + 48 * n
        feats = r.readback_features()
        r.render(5, 3)
        r.render_features(5, 0)  # nothing to add, nothing allocated
        assert r.stats().device_bytes == before + 48 * n
        img, samples = r.readback(), r.stats().samples
        assert_same(r.readback_features(), feats, "after pt_render")
        r.clear()
        assert not bits(r.readback()).any()
        cleared = r.readback_features()
        assert all(not bits(cleared[k]).any() for k in KEYS)
        r.render_features(1, 4)
        assert_same(r.readback_features(), feats, "after pt_clear")
    finally:
        r.free()
    r = capi.Renderer(capi.Scene(path, res=RES), **kw)
    try:
        r.render(1, 4)
        r.render(5, 3)
        assert np.array_equal(bits(r.readback()), bits(img))
        assert r.stats().samples == samples == 7 * n
    finally:
        r.free()


def test_errors(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(32, 24)))
    try:
        with pytest.raises(capi.PtError, match="no feature pass"):
            r.readback_features()
        with pytest.raises(capi.PtError):
            r.render_features(0, 1)
        with pytest.raises(capi.PtError):
            r.render_features(1, -1)
        with pytest.raises(capi.PtError, match="no feature pass"):
            r.readback_features()  # a refused call allocates nothing
        r.render_features(3, 0)  # no iterations: allocates the zeroed buffers and nothing else
        empty = r.readback_features()
        assert all(not bits(empty[k]).any() for k in KEYS) and empty["object_id"].shape == (32 * 24,)
    finally:
        r.free()


def test_group_gather_equals_single_context(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path, res = scene_dir["cornell"], (96, 60)
    single = features(path, res, ((1, 3),), aa_jitter=True)
    g = capi.Group(capi.Scene(path, res=res), [0, 0, 0], aa_jitter=True)
    try:
        assert g.transport == "copy"
        with pytest.raises(capi.PtError):
            g.gather_features()
        g.render_features(1, 3)
        got = g.gather_features()
    finally:
        g.free()
    assert_same(got, single, "three contexts on one device")
