"""Retirement records at fixed slots, gathered as a stream (csrc/pt_sched.h fixed_slots, DESIGN.md sections 4 and 5).

In a first-bounce batch record i of sub-list (q, k, rho) is the same pixel for every k, so k_paths stores a path's retirement record
at the slot its list position gives instead of at the next free slot of its visit, and the gather (k_collect_stream) adds the K
records of a slot in iteration order, one thread per slot, without a tile.  Which slot a record lies in changes no sample and no
order of summation: the image, the live-ray counts and the sample count must be, bit for bit and in exact, fma and fast, those of
  16384  records in order of retirement under the tile gather (the code as it was),
  32768  fixed slots under the tile gather, which places a record by its pixel word — a second, independent check of the stores,
  8192   split records,
and in exact mode all of them are the oracle's image.  PtStats.gather_form says how a context's last batch was gathered.

Every render runs on a FRESH context: the record buffer starts as NaN colours, so a slot nobody wrote shows in the first batch."""
import numpy as np
import pytest

from test_gpu_first_hit_sharing import assert_is_oracle, bits
from test_gpu_retire_once import _oracle_tile, _scene, _stripes

pytestmark = pytest.mark.gpu
BY_VISIT, TILE_GATHER, SPLIT_RECORDS = 16384, 32768, 8192  # PtOptions.debug_flags
TILE, TILE_FIXED, STREAM = 0, 1, 2                         # PtStats.gather_form
FIRST, SPLIT = 2, 1                                        # PtStats.record_form
ARITHS = ["exact", "fma", "fast"]
# (arm, debug_flags, record form, gather form)
ARMS = (("default", 0, FIRST, STREAM), ("by visit", BY_VISIT, FIRST, TILE), ("tile gather", TILE_GATHER, FIRST, TILE_FIXED),
        ("split records", SPLIT_RECORDS, SPLIT, TILE))


def render_in_calls(path, res, calls, **kw):
    """(image, stats) after the render calls `calls` = [(first iteration, count), ...] on one fresh context."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(path, res=res), **kw)
    try:
        for first, count in calls:
            r.render(first, count)
        return r.readback(), r.stats()
    finally:
        r.free()


def four_arms(path, res, calls, arith, **kw):
    """The default image, after asserting that every arm ran the forms its switch asks for and gave the same image, samples and rays."""
    spp = sum(count for _, count in calls)
    out = {name: render_in_calls(path, res, calls, arith=arith, debug_flags=flags, **kw) for name, flags, _, _ in ARMS}
    img, st = out["default"]
    assert np.isfinite(img).all(), f"{arith}: {(~np.isfinite(img)).any(axis=1).sum()} pixels of the default image are not finite"
    for name, _, record_form, gather_form in ARMS:
        other, st_o = out[name]
        assert (st_o.record_form, st_o.gather_form) == (record_form, gather_form), f"{name}: forms {st_o.record_form}, {st_o.gather_form}"
        assert np.isfinite(other).all(), name
        diff = (bits(img) != bits(other)).any(axis=1)
        assert not diff.any(), f"{arith}: {diff.sum()} pixels differ from the '{name}' image, first {np.flatnonzero(diff)[:8]}"
        assert st.samples == st_o.samples == img.shape[0] * spp
        assert list(st.live_rays) == list(st_o.live_rays)
    return img, st


# (id, scene, resolution, render calls, trace depth, renderer options)
CASES = [
    # batches of 3, 3 and 1: full batches and a partial one
    ("cornell, batches of 3", "cornell", (96, 64), [(1, 7)], 8, dict(iters_per_batch=3)),
    # the same seven iterations in two calls into one image: batches of 3 + 1, then 3
    ("two render calls", "cornell", (96, 64), [(1, 4), (5, 3)], 8, dict(iters_per_batch=3)),
    ("gap slots", "cornell", (97, 61), [(1, 7)], 8, dict(iters_per_batch=3)),  # 5917 pixels: the tile's last chunk has 29
    ("depth 2", "cornell", (96, 64), [(1, 5)], 2, dict(iters_per_batch=3)),  # every path dies in the round after it was taken
    ("70 iterations in one batch", "cornell", (96, 64), [(1, 70)], 8, dict(iters_per_batch=70)),  # k_primary's runs longer than 64
    # 26 leaves (the top list holds 32: tables in LDS), mirrors and partly reflective materials among the twenty objects
    ("random scene", "random20", (96, 64), [(1, 6)], 8, dict(iters_per_batch=4)),
    # fewer pixels than a wave has lanes, across the box's edge (nine pixels beside it, the others inside): sub-lists of a path or two,
    # dozens of visits per refill — what the visit ring's lap guard existed for
    ("tile of 40 pixels", "cornell", (96, 64), [(1, 40)], 8, dict(iters_per_batch=40, pixel_begin=32 * 96 + 10, pixel_count=40)),
    ("rank 3 of 8, striped", "cornell", (96, 64), [(1, 40)], 8, dict(iters_per_batch=40, **_stripes(96, 64, 3, 8))),
    # one queue owns all 24,000 pixels: more than a pass of the tile gather holds (8192); the stream has no passes, 94 blocks for the queue
    ("one queue", "cornell", (200, 120), [(1, 5)], 8, dict(iters_per_batch=3, num_queues=1)),
]

_refs = {}


def _path(scene, depth, res, scene_dir, tmp):
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    if scene == "random20":
        return scenes.write_scene(scenes.random_scene_text(2, 20, res=res, depth=depth), str(tmp / "random20.txt"))
    return _scene(scene, depth, res, scene_dir, tmp)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name,scene,res,calls,depth,kw", CASES, ids=[c[0] for c in CASES])
def test_same_image_in_every_arm(scene_dir, oracle, tmp_path_factory, name, scene, res, calls, depth, kw, arith):
    path = _path(scene, depth, res, scene_dir, tmp_path_factory.mktemp("fixed_slots"))
    img, st = four_arms(path, res, calls, arith, **kw)
    assert 0 < st.live_rays[1] < st.samples  # some samples survive depth 0 and some do not: survivor slots and retiree slots exist
    if arith == "exact":
        spp = sum(count for _, count in calls)
        key = (scene, res, spp, depth, tuple(sorted((k, v) for k, v in kw.items() if k != "iters_per_batch")))
        if key not in _refs:  # (computed once, read only; the two cornell 96x64 cases of seven iterations share one)
            _refs[key] = _oracle_tile(oracle, path, res, spp, depth, kw)
        assert_is_oracle([img], _refs[key])


def test_the_random_scene_has_mirrors_and_partly_reflective_objects(tmp_path):
    """The case above holds what it says, by the scene's own description."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    sc = capi.Scene(_path("random20", 8, (96, 64), {}, tmp_path), res=(96, 64))
    used = {int(sc.desc.geoms[i].materialid) for i in range(sc.desc.num_geoms)}
    refl = {float(sc.desc.materials[m].hasReflective) for m in used}
    assert 1.0 in refl and any(0.0 < r < 1.0 for r in refl) and 0.0 in refl
    assert sc.desc.num_geoms <= 32


@pytest.mark.parametrize("arith", ARITHS)
def test_convergence_gather(scene_dir, arith):
    """The metric's batches keep the tile gather (its partial sums have a fixed partition) over fixed-slot records; the batches before
    the capture stream.  Image and per-iteration squared errors must be those of records by visit: reference frame captured in the
    second batch, so batches before, at and after the capture are gathered."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res, iters = (97, 61), 12

    def run(flags):
        r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=res), convergence=7, iters_per_batch=5, arith=arith, debug_flags=flags)
        try:
            r.render(1, 5)
            first = r.stats().gather_form
            r.render(6, iters - 5)
            return r.convergence(1, iters), r.readback(), (first, r.stats().gather_form)
        finally:
            r.free()

    sse, img, forms = run(0)
    sse_v, img_v, forms_v = run(BY_VISIT)
    assert forms == (STREAM, TILE_FIXED) and forms_v == (TILE, TILE)
    assert np.isfinite(img).all() and np.array_equal(bits(img), bits(img_v))
    assert np.array_equal(sse.view(np.uint64), sse_v.view(np.uint64)) and (sse[7:] > 0).all()
