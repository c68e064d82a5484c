"""The first bounce sampled in k_paths, k_primary once per batch (csrc/pt_sched.h first_bounces, DESIGN.md sections 4 and 5).

In a batch that splits its records everything depth 0 does per iteration for a surviving pixel is a function of its first hit and
the iteration.  On scenes whose tables the fused kernels keep in LDS k_primary therefore traces a chunk once per batch and writes
ONE record per surviving pixel (bounce origin, hit normal, camera direction, pixel | material); the lane of k_paths that takes the
record for iteration k draws that iteration's specular / diffuse choice, forms the throughput and samples the first bounce.
Nothing about the samples changes, so the image, the live-ray counts and the sample count must be those of split records
(PtOptions.debug_flags 8192), of whole records (4096) and of the per-iteration form (128), bit for bit, in exact, fma and fast —
and in exact mode all four are the oracle's image.  PtStats.record_form says which form a context's last batch ran.

Every render runs on a FRESH context: the path buffers are filled with NaN when they are allocated, so a record nobody wrote in
this batch has a NaN origin, which the comparisons see in the first batch."""
import numpy as np
import pytest

from test_gpu_first_hit_sharing import assert_is_oracle, bits, gpu_render
from test_gpu_retire_once import _oracle_tile, _scene, _stripes
from test_gpu_split_records import _half_mirror_text

pytestmark = pytest.mark.gpu
SPLIT_RECORDS = 8192  # PtOptions.debug_flags: split records where the default samples the first bounce in k_paths
WHOLE_RECORDS = 4096  # whole 40-byte depth-1 records in every iteration
PER_ITERATION = 128   # depth 0 traced in every iteration (which writes whole records too)
WHOLE, SPLIT, FIRST = 0, 1, 2  # PtStats.record_form
ARITHS = ["exact", "fma", "fast"]


def four_ways(path, res, spp, arith, form, **kw):
    """The default render, after asserting that it ran record form `form` and that the batches with bit 8192, with bit 4096 and
    the per-iteration form — each in the form its switch asks for — give the same image, samples and live rays."""
    flags = kw.pop("debug_flags", 0)
    arms = (("default", 0, form), ("split records", SPLIT_RECORDS, min(form, SPLIT)), ("whole records", WHOLE_RECORDS, WHOLE), ("per iteration", PER_ITERATION, WHOLE))
    out = {name: gpu_render(path, res, spp, arith=arith, debug_flags=flags | extra, **kw) for name, extra, _ in arms}  # a fresh context each
    img, st = out["default"]
    assert np.isfinite(img).all(), f"{arith}: {(~np.isfinite(img)).any(axis=1).sum()} pixels of the default image are not finite"
    for name, _, want in arms:
        other, st_o = out[name]
        assert st_o.record_form == want, f"{name}: record form {st_o.record_form}, expected {want}"
        assert np.isfinite(other).all(), name
        diff = (bits(img) != bits(other)).any(axis=1)
        assert not diff.any(), f"{arith}: {diff.sum()} pixels differ from the '{name}' image, first {np.flatnonzero(diff)[:8]}"
        assert st.samples == st_o.samples == img.shape[0] * spp
        assert list(st.live_rays) == list(st_o.live_rays)
    return img, st


# (id, scene, resolution, iterations, trace depth, renderer options, record form of the default render)
CASES = [
    ("cornell 16:9", "cornell", (208, 117), 7, 8, dict(iters_per_batch=3), FIRST),
    ("partial last chunk", "cornell", (201, 119), 3, 8, {}, FIRST),  # 23919 pixels: the tile's last chunk has 47
    ("one iteration per batch", "cornell", (96, 64), 3, 8, dict(iters_per_batch=1), FIRST),
    ("batches of 7, then 3", "cornell", (96, 64), 10, 8, dict(iters_per_batch=7), FIRST),
    ("sphere", "sphere", (96, 64), 4, 8, {}, FIRST),
    ("depth 2", "cornell", (96, 64), 5, 2, dict(iters_per_batch=3), FIRST),  # a path lives exactly one bounce: the one sampled at the take
    ("depth 1: the rule is off", "cornell", (96, 64), 5, 1, dict(iters_per_batch=3), WHOLE),
    ("aa_jitter: the rule is off", "cornell", (96, 64), 5, 8, dict(iters_per_batch=3, aa_jitter=True), WHOLE),
    ("striped tile", "cornell", (192, 108), 5, 8, dict(iters_per_batch=3, **_stripes(192, 108, 0, 8)), FIRST),
    ("one queue", "cornell", (200, 120), 5, 8, dict(iters_per_batch=3, num_queues=1), FIRST),
    # the search forms whose next record waits in registers keep split records
    ("packet scan", "random", (96, 64), 6, 8, dict(iters_per_batch=4, lds_table_kb=-1, debug_flags=512), SPLIT),
    ("grid forced", "random", (96, 64), 6, 8, dict(iters_per_batch=4, lds_table_kb=-1, debug_flags=256), SPLIT),
    # the specular draw now happens in k_paths, once per iteration of a pixel: a constant kind cannot give the oracle's image
    ("half mirror", "half mirror", (96, 64), 8, 8, dict(iters_per_batch=8), FIRST),
    # the form traces once per batch whatever the pieces and the share say
    ("pieces and share ignored", "cornell", (96, 64), 11, 8, dict(iters_per_batch=9, primary_share=2, primary_pieces=2), FIRST),
    # K > 64: the count store loops over the lanes, and k needs more than six bits beside the visit number
    ("70 iterations in one batch", "cornell", (96, 64), 70, 8, dict(iters_per_batch=70), FIRST),
    # an eighth of a small frame in stripes, 40 iterations: sub-lists of a path or two, several visits per refill — the visit-lap
    # guard on the packed visit word
    ("tiny sub-lists", "cornell", (96, 64), 40, 8, dict(iters_per_batch=40, **_stripes(96, 64, 0, 8)), FIRST),
    # pieces of a path or more: piece switches while taken lanes are in flight, last rounds with nothing left to take
    ("many pieces", "cornell", (96, 64), 5, 8, dict(iters_per_batch=3, paths_pieces=4, paths_min_piece=1), FIRST),
    # triangles: the one record per pixel stores a triangle's FINISHED normal where the other types store theirs.  scenes.mesh_scene_text
    # has 26 leaves, which fit the top list, so its tables are in LDS (search form 0, pt_lds.h), and pt_sched.h first_bounces holds:
    # shared depth 0, no jitter, depth 8, five materials, K = 3 (the sweep of tests/sched_first_bounce_driver.cpp: record_form=2)
    ("mesh", "mesh", (96, 64), 5, 8, dict(iters_per_batch=3), FIRST),
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
@pytest.mark.parametrize("name,scene,res,spp,depth,kw,form", CASES, ids=[c[0] for c in CASES])
def test_same_image_four_ways(scene_dir, oracle, tmp_path_factory, name, scene, res, spp, depth, kw, form, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    tmp = tmp_path_factory.mktemp("first_bounce")
    if scene == "mesh":
        path = scenes.write_scene(scenes.mesh_scene_text(res=res, depth=depth), str(tmp / "mesh.txt"))
    else:
        path = scenes.write_scene(_half_mirror_text(), str(tmp / "half_mirror.txt")) if scene == "half mirror" else _scene(scene, depth, res, scene_dir, tmp)
    img, st = four_ways(path, res, spp, arith, form, **kw)
    if scene in ("cornell", "half mirror", "mesh") and depth >= 2:
        assert 0 < st.live_rays[1] < st.samples  # some samples survive depth 0 and some do not: depth-1 records exist
    if name == "packet scan":
        assert st.grid_cells == 0
    if name == "grid forced":
        assert st.grid_cells > 0  # the grid is what was walked
    if arith == "exact":
        assert_is_oracle([img], _reference(oracle, name, path, res, spp, depth, kw))


@pytest.mark.parametrize("arith", ARITHS)
def test_stale_records_are_not_read(scene_dir, arith):
    """A context whose path buffers hold another batch split's records (a batch of 4, then — after clear — batches of 7 and 3)
    renders what a fresh context renders, with the rule on and with bit 8192."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res, spp = (208, 117), 10
    fresh, st_f = gpu_render(scene_dir["cornell"], res, spp, arith=arith, iters_per_batch=7)
    split, st_s = gpu_render(scene_dir["cornell"], res, spp, arith=arith, iters_per_batch=7, debug_flags=SPLIT_RECORDS)
    assert st_f.record_form == FIRST and st_s.record_form == SPLIT
    assert np.isfinite(fresh).all() and np.array_equal(bits(split), bits(fresh))
    for flags, form in ((0, FIRST), (SPLIT_RECORDS, SPLIT)):
        r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=res), arith=arith, iters_per_batch=7, debug_flags=flags)
        try:
            r.render(1, 4)
            r.clear()
            r.render(1, spp)
            again, st = r.readback(), r.stats()
        finally:
            r.free()
        assert st.record_form == form
        assert np.isfinite(again).all() and np.array_equal(bits(again), bits(fresh))
        assert st.samples == st_f.samples == st_s.samples and list(st.live_rays) == list(st_f.live_rays) == list(st_s.live_rays)
