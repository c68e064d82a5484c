"""The iteration-invariant half of a depth-1 record written once per batch (csrc/pt_sched.h splits_records).

In the shared form with depth >= 2 the pixels that survive depth 0 are the same in every iteration, and so are the origin of
their bounce ray and the material they hit: k_primary writes (origin, material) once per batch, at the slot the pixel's record
has in iteration 0, and per iteration only (direction, sample id | specular bit); k_paths reads both words and forms the
throughput from its material table.  Nothing about the samples changes, so the image, the live-ray counts and the sample count
must be those of the batch with whole records (PtOptions.debug_flags 4096) and of the per-iteration form (128), bit for bit, in
exact, fma and fast — and in exact mode all three are the oracle's image.

Every render runs on a FRESH context: the path buffers are filled with NaN when they are allocated, so a record whose invariant
half nobody wrote in this batch has a NaN origin and an undefined material, which the comparisons see in the first batch."""
import numpy as np
import pytest

from test_gpu_first_hit_sharing import assert_is_oracle, bits, gpu_render
from test_gpu_retire_once import _oracle_tile, _scene, _stripes

pytestmark = pytest.mark.gpu
WHOLE_RECORDS = 4096  # PtOptions.debug_flags: whole 40-byte depth-1 records in every iteration
PER_ITERATION = 128   # PtOptions.debug_flags: depth 0 traced in every iteration (which writes whole records too)
ARITHS = ["exact", "fma", "fast"]


def three_ways(path, res, spp, arith, **kw):
    """The default render, after asserting that the batch with bit 4096 and the per-iteration form give the same one."""
    flags = kw.pop("debug_flags", 0)
    out = {}
    for name, extra in (("default", 0), ("whole records", WHOLE_RECORDS), ("per iteration", PER_ITERATION)):
        out[name] = gpu_render(path, res, spp, arith=arith, debug_flags=flags | extra, **kw)  # a fresh context each
    img, st = out["default"]
    assert np.isfinite(img).all(), f"{arith}: {(~np.isfinite(img)).any(axis=1).sum()} pixels of the default image are not finite"
    for name in ("whole records", "per iteration"):
        other, st_o = out[name]
        assert np.isfinite(other).all(), name
        diff = (bits(img) != bits(other)).any(axis=1)
        assert not diff.any(), f"{arith}: {diff.sum()} pixels differ from the '{name}' image, first {np.flatnonzero(diff)[:8]}"
        assert st.samples == st_o.samples == img.shape[0] * spp
        assert list(st.live_rays) == list(st_o.live_rays)
    return img, st


def _half_mirror_text(depth=8):
    """cornell.txt with a sphere that reflects half of the time and whose two colours differ: a pixel on it is specular in some
    iterations and diffuse in others, with another throughput."""
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    text = scenes.cornell_scene_text(depth=depth)
    head, sep, tail = text.partition("MATERIAL 4\n")
    assert sep and tail.count("REFL        1\n") == 1 and tail.startswith("RGB         .98 .98 .98\n")
    tail = tail.replace("RGB         .98 .98 .98\n", "RGB         .35 .35 .85\n", 1).replace("REFL        1\n", "REFL        0.5\n", 1)
    return head + sep + tail


# (id, scene, resolution, iterations, trace depth, renderer options)
CASES = [
    ("cornell 16:9", "cornell", (208, 117), 7, 8, dict(iters_per_batch=3)),
    ("sphere", "sphere", (96, 64), 4, 8, {}),
    ("partial last chunk", "cornell", (201, 119), 3, 8, {}),  # 23919 pixels: the tile's last chunk has 47
    ("one iteration per batch", "cornell", (96, 64), 3, 8, dict(iters_per_batch=1)),
    ("batches of 7, then 3", "cornell", (96, 64), 10, 8, dict(iters_per_batch=7)),
    # batches of 9 in pieces of 5 + 4, runs of at most 2: only the first sub-run of the first piece holds iteration 0, so every
    # other run's records find their invariant halves written by another wave
    ("two pieces, several sub-runs", "cornell", (96, 64), 11, 8, dict(iters_per_batch=9, primary_share=2, primary_pieces=2)),
    ("depth 2", "cornell", (96, 64), 5, 2, dict(iters_per_batch=3)),  # a path lives exactly one bounce on its depth-1 record
    ("depth 1: the rule is off", "cornell", (96, 64), 5, 1, dict(iters_per_batch=3)),
    ("aa_jitter: the rule is off", "cornell", (96, 64), 5, 8, dict(iters_per_batch=3, aa_jitter=True)),
    ("striped tile", "cornell", (192, 108), 5, 8, dict(iters_per_batch=3, **_stripes(192, 108, 0, 8))),
    ("one queue", "cornell", (200, 120), 5, 8, dict(iters_per_batch=3, num_queues=1)),
    ("packet scan", "random", (96, 64), 6, 8, dict(iters_per_batch=4, lds_table_kb=-1, debug_flags=512)),  # k_paths mode 1
    ("grid forced", "random", (96, 64), 6, 8, dict(iters_per_batch=4, lds_table_kb=-1, debug_flags=256)),  # k_paths mode 2
    # the kind bit differs between the iterations of one pixel: a constant bit cannot give the oracle's image
    ("half mirror", "half mirror", (96, 64), 8, 8, dict(iters_per_batch=8)),
]

_refs = {}


def _reference(oracle, name, path, res, spp, depth, kw):
    if name not in _refs:  # (computed once, read only)
        try:
            oracle.set_aa_jitter(bool(kw.get("aa_jitter")))
            _refs[name] = _oracle_tile(oracle, path, res, spp, depth, kw)
        finally:
            oracle.set_aa_jitter(False)
    return _refs[name]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name,scene,res,spp,depth,kw", CASES, ids=[c[0] for c in CASES])
def test_same_image_three_ways(scene_dir, oracle, tmp_path_factory, name, scene, res, spp, depth, kw, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    tmp = tmp_path_factory.mktemp("split_records")
    path = scenes.write_scene(_half_mirror_text(), str(tmp / "half_mirror.txt")) if scene == "half mirror" else _scene(scene, depth, res, scene_dir, tmp)
    img, st = three_ways(path, res, spp, arith, **kw)
    if scene in ("cornell", "half mirror") and depth >= 2 and not kw.get("pixel_count"):
        assert 0 < st.live_rays[1] < st.samples  # some samples survive depth 0 and some do not: depth-1 records exist
    if name == "packet scan":
        assert st.grid_cells == 0
    if name == "grid forced":
        assert st.grid_cells > 0  # the grid is what was walked
    if arith == "exact":
        assert_is_oracle([img], _reference(oracle, name, path, res, spp, depth, kw))


def test_the_half_mirror_changes_its_mind(oracle, tmp_path):
    """The last case above holds what it says, by the oracle alone: with trace depth 1 a sample retires at depth 0 with exactly
    the throughput a deeper path would carry on — the sphere's spec (.98 grey) or its color (.35, .35, .85) — and there are pixels
    that show both within the case's 8 iterations."""
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    res = (96, 64)
    path = scenes.write_scene(_half_mirror_text(depth=1), str(tmp_path / "half_mirror_d1.txt"))
    oracle.set_math_mode(oracle.PORTABLE)
    oracle.load_scene(path, res=res)
    frames = np.stack([oracle.render(i, 1, depth=1, variant=oracle.RETIRE, nthreads=16).reshape(-1, 3) for i in range(1, 9)])
    grey, blue = np.float32([.98, .98, .98]), np.float32([.35, .35, .85])
    specular, diffuse = (frames == grey).all(axis=2), (frames == blue).all(axis=2)
    assert (specular.any(axis=0) & diffuse.any(axis=0)).sum() >= 10


@pytest.mark.parametrize("arith", ARITHS)
def test_stale_invariant_halves_are_not_read(scene_dir, arith):
    """A context whose path buffers hold another batch split's records (a batch of 4, then — after clear — batches of 7 and 3)
    renders what a fresh context renders, with the rule on and with it off."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res, spp = (208, 117), 10
    fresh, st_f = gpu_render(scene_dir["cornell"], res, spp, arith=arith, iters_per_batch=7)
    whole, st_w = gpu_render(scene_dir["cornell"], res, spp, arith=arith, iters_per_batch=7, debug_flags=WHOLE_RECORDS)
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=res), arith=arith, iters_per_batch=7)
    try:
        r.render(1, 4)
        r.clear()
        r.render(1, spp)
        again, st = r.readback(), r.stats()
    finally:
        r.free()
    assert np.isfinite(again).all() and np.array_equal(bits(again), bits(fresh)) and np.array_equal(bits(whole), bits(fresh))
    assert st.samples == st_f.samples == st_w.samples and list(st.live_rays) == list(st_f.live_rays) == list(st_w.live_rays)
