"""Depth-0 retirees stored and gathered once per batch (csrc/pt_sched.h retires_once).

In the shared form with depth >= 2 a camera ray that misses the scene or hits an emitter retires at depth 0 in every iteration
with the same colour, so k_primary writes its record in iteration 0 of a batch only and k_collect gathers it there only; the
LDS tile keeps the pixel's colour for the other iterations.  Nothing about the samples changes, so the image, the live-ray
counts and the sample count must be those of the batch that stores and gathers every record (PtOptions.debug_flags 1024) and
of the per-iteration form (128), bit for bit, in exact, fma and fast — and in exact mode all three are the oracle's image.

Every render runs on a FRESH context: the record buffer is filled with NaN when it is allocated, so a gather that read a slot
nobody wrote in this batch puts NaN into the first batch's image, which the finiteness check and every comparison see."""
import numpy as np
import pytest

from test_gpu_first_hit_sharing import assert_is_oracle, bits, gpu_render

pytestmark = pytest.mark.gpu
EVERY_ITERATION = 1024  # PtOptions.debug_flags: depth-0 retirees stored and gathered in every iteration
PER_ITERATION = 128     # PtOptions.debug_flags: depth 0 traced in every iteration (which stores every record too)
ARITHS = ["exact", "fma", "fast"]


def _scene(name, depth, res, scene_dir, tmp):
    """Path of the scene `name` with trace depth `depth` (conftest's scenes have depth 8)."""
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    if depth == 8 and name in scene_dir:
        return scene_dir[name]
    if name == "random":  # 33 leaves: more than the top list holds (tests/test_gpu_first_hit_sharing.py)
        return scenes.write_scene(scenes.random_scene_text(2, 27, res=res, depth=depth), str(tmp / "random.txt"))
    text = {"cornell": scenes.cornell_scene_text, "sphere": scenes.sphere_scene_text}[name](depth=depth)
    return scenes.write_scene(text, str(tmp / f"{name}_d{depth}.txt"))


def _oracle_tile(oracle, path, res, spp, depth, kw):
    """The oracle's image (PORTABLE math, RETIRE loop) of the tile the renderer options `kw` select, in tile order."""
    w, h = res
    oracle.set_math_mode(oracle.PORTABLE)
    oracle.load_scene(path, res=res)
    run = lambda begin, count: oracle.render(1, spp, depth=depth, variant=oracle.RETIRE, nthreads=16, pix_begin=begin, pix_count=count).reshape(-1, 3)
    begin, count = kw.get("pixel_begin", 0), kw.get("pixel_count", 0) or w * h - kw.get("pixel_begin", 0)
    stripe, stride = kw.get("stripe_pixels", 0), kw.get("stripe_stride", 0)
    if not stripe:
        return run(begin, count)
    return np.concatenate([run(begin + i * stride, stripe) for i in range(count // stripe)])


def three_ways(path, res, spp, arith, **kw):
    """The default image, after asserting that the batch with bit 1024 and the per-iteration form give the same one."""
    flags = kw.pop("debug_flags", 0)
    out = {}
    for name, extra in (("default", 0), ("every iteration", EVERY_ITERATION), ("per iteration", PER_ITERATION)):
        out[name] = gpu_render(path, res, spp, arith=arith, debug_flags=flags | extra, **kw)  # a fresh context each
    img, st = out["default"]
    assert np.isfinite(img).all(), f"{arith}: {(~np.isfinite(img)).any(axis=1).sum()} pixels of the default image are not finite"
    for name in ("every iteration", "per iteration"):
        other, st_o = out[name]
        assert np.isfinite(other).all(), name
        diff = (bits(img) != bits(other)).any(axis=1)
        assert not diff.any(), f"{arith}: {diff.sum()} pixels differ from the '{name}' image, first {np.flatnonzero(diff)[:8]}"
        assert st.samples == st_o.samples == img.shape[0] * spp
        assert list(st.live_rays) == list(st_o.live_rays)
    return img, st


def _stripes(w, h, rank, world):
    from cosc_4397_pathtracing_raytracing_project_amd import parallel
    return parallel.striped_tile_for_rank(w, h, rank, world)


# (id, scene, resolution, iterations, trace depth, renderer options)
CASES = [
    # 16:9: runs of 64 and more pixels beside the box (whole chunks retire at depth 0), chunks across its edge, the light in view
    ("cornell 16:9", "cornell", (208, 117), 7, 8, dict(iters_per_batch=3)),
    ("sphere", "sphere", (96, 64), 4, 8, {}),
    ("partial last chunk", "cornell", (201, 119), 3, 8, {}),  # 23919 pixels: the tile's last chunk has 47
    ("one iteration per batch", "cornell", (96, 64), 3, 8, dict(iters_per_batch=1)),
    ("batches of 2, then 1", "cornell", (96, 64), 5, 8, dict(iters_per_batch=2)),
    ("batches of 7, then 3", "cornell", (96, 64), 10, 8, dict(iters_per_batch=7)),
    # batches of 9 in pieces of 5 + 4, runs of at most 2: sub-runs 2 + 2 + 1 and 2 + 2; only the very first holds iteration 0
    ("two pieces, several sub-runs", "cornell", (96, 64), 11, 8, dict(iters_per_batch=9, primary_share=2, primary_pieces=2)),
    ("depth 1: the rule is off", "cornell", (96, 64), 5, 1, dict(iters_per_batch=3)),  # every sample retires at depth 0, by a draw
    ("depth 2", "cornell", (96, 64), 5, 2, dict(iters_per_batch=3)),
    ("depth 8", "cornell", (96, 64), 5, 8, dict(iters_per_batch=3)),
    ("striped tile", "cornell", (192, 108), 5, 8, dict(iters_per_batch=3, **_stripes(192, 108, 1, 4))),
    ("small tile", "cornell", (192, 108), 5, 8, dict(iters_per_batch=3, pixel_begin=9001, pixel_count=777)),
    ("grid forced", "stress_big", (160, 90), 4, 8, dict(debug_flags=256)),
    ("packet scan", "random", (96, 64), 6, 8, dict(iters_per_batch=4, lds_table_kb=-1, debug_flags=512)),
    # one queue owns all 24,000 pixels: more than the gather's 8192 per pass — three passes, each over a region of three chunks
    ("one queue, three passes", "cornell", (200, 120), 5, 8, dict(iters_per_batch=3, num_queues=1)),
]

_refs = {}


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name,scene,res,spp,depth,kw", CASES, ids=[c[0] for c in CASES])
def test_same_image_three_ways(scene_dir, oracle, tmp_path_factory, name, scene, res, spp, depth, kw, arith):
    path = _scene(scene, depth, res, scene_dir, tmp_path_factory.mktemp("retire_once"))
    img, st = three_ways(path, res, spp, arith, **kw)
    if scene == "cornell" and depth >= 2 and not kw.get("pixel_count"):
        assert 0 < st.live_rays[1] < st.samples  # some samples retire at depth 0 and some do not: both kinds of slot exist
    if arith == "exact":
        if name not in _refs:  # (computed once, read only)
            _refs[name] = _oracle_tile(oracle, path, res, spp, depth, kw)
        assert_is_oracle([img], _refs[name])


def test_whole_chunks_retire_in_the_wide_frame(scene_dir, oracle):
    """The first case above holds what it says: 64-pixel chunks (pixels 64 g .. 64 g + 63) every pixel of which misses the scene or
    sees the light, chunks with both kinds of pixel, and chunks where every pixel bounces on — by the oracle, no GPU involved."""
    res = (208, 117)
    oracle.set_math_mode(oracle.PORTABLE)
    oracle.load_scene(scene_dir["cornell"], res=res)
    # a pixel retires at depth 0 exactly when its colour does not depend on the iteration: three iterations, one at a time
    a = oracle.render(1, 1, depth=2, variant=oracle.RETIRE, nthreads=16).reshape(-1, 3)
    b = oracle.render(2, 1, depth=2, variant=oracle.RETIRE, nthreads=16).reshape(-1, 3)
    c = oracle.render(3, 1, depth=2, variant=oracle.RETIRE, nthreads=16).reshape(-1, 3)
    fixed = ((bits(a) == bits(b)) & (bits(a) == bits(c))).all(axis=1)  # (a bouncing pixel repeats itself three times with negligible probability)
    n = fixed.size // 64 * 64
    per_chunk = fixed[:n].reshape(-1, 64).sum(axis=1)
    assert (per_chunk == 64).sum() >= 10 and (per_chunk == 0).sum() >= 1 and ((per_chunk > 0) & (per_chunk < 64)).sum() >= 10


@pytest.mark.parametrize("arith", ARITHS)
def test_convergence_gather(scene_dir, arith):
    """k_collect_conv shares the gather's body: image and squared errors with and without bit 1024, reference frame captured in the
    second batch (so batches before, at and after the capture are gathered)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res, iters = (200, 120), 12

    def run(flags):
        r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=res), convergence=7, iters_per_batch=5, arith=arith, debug_flags=flags)
        try:
            r.render(1, iters)
            return r.convergence(1, iters), r.readback()
        finally:
            r.free()

    sse, img = run(0)
    sse_every, img_every = run(EVERY_ITERATION)
    assert np.isfinite(img).all() and np.array_equal(bits(img), bits(img_every))
    assert np.array_equal(sse.view(np.uint64), sse_every.view(np.uint64)) and (sse[7:] > 0).all()


@pytest.mark.parametrize("arith", ARITHS)
def test_clear_then_render_again(scene_dir, arith):
    """A second render on a context whose record buffer holds the first one's records is a fresh context's render."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res, spp = (208, 117), 5
    fresh, st_f = gpu_render(scene_dir["cornell"], res, spp, arith=arith, iters_per_batch=3)
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=res), arith=arith, iters_per_batch=3)
    try:
        r.render(1, 4)  # another batch split: 3 + 1
        r.clear()
        r.render(1, spp)
        again, st = r.readback(), r.stats()
    finally:
        r.free()
    assert np.isfinite(again).all() and np.array_equal(bits(again), bits(fresh))
    assert st.samples == st_f.samples and list(st.live_rays) == list(st_f.live_rays)
