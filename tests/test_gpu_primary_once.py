"""Depth 0 traced once per camera (csrc/pt_sched.h primary_once, DESIGN.md sections 4 and 5).

In a first-bounce batch with fixed record slots what k_primary leaves behind — one record per surviving pixel, the depth-0 retirees'
records, the pair of counts of every sub-list — depends on the camera, the tables, the tile and the plan, not on the batch.  The
host therefore launches the kernel in the first such batch after pt_init or pt_set_camera and again only when one of those inputs
has changed; later batches read what it left, and k_paths writes the counter row of depth 0 that the statistics read and re-zero.
PtOptions.debug_flags 65536 launches it in every batch, as it was.  Nothing about the samples changes, so every sequence below gives
the same images, samples and live rays with and without the bit, bit for bit, in exact, fma and fast — and in exact mode the
oracle's image.  PtStats.primary_launches shows the launches saved.

Iterations come in batches of 3 (iters_per_batch), so ten of them are batches of 3, 3, 3 and 1."""
import numpy as np
import pytest

from test_gpu_first_hit_sharing import assert_is_oracle, bits
from test_gpu_retire_once import _oracle_tile

pytestmark = pytest.mark.gpu
EVERY_BATCH = 65536   # PtOptions.debug_flags: k_primary in every batch
SPLIT_RECORDS, BY_VISIT = 8192, 16384  # ... split records instead of the first bounce in k_paths; records in order of retirement
ARITHS = ["exact", "fma", "fast"]
FRAMES = [((96, 64), 8), ((64, 48), 2)]  # (resolution, trace depth)
FRAME_IDS = ["96x64 depth 8", "64x48 depth 2"]
FIRST = 2  # PtStats.record_form


def _two_axes_text(depth):
    """cornell.txt with a left wall that reflects half of the time around a narrowed lobe: the sphere stays the rough mirror it is
    (REFL 1, roughness 1 - REFR = 1), so a wave holds specular takes, whose axis is the reflected camera direction, beside diffuse
    takes on the same material and on the others, whose axis is the normal."""
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    text = scenes.cornell_scene_text(depth=depth)
    head, sep, tail = text.partition("MATERIAL 2\n")
    assert sep and tail.startswith("RGB         .85 .35 .35\nSPECEX      0\nSPECRGB     0 0 0\nREFL        0\nREFR        0\n")
    tail = tail.replace("SPECRGB     0 0 0\nREFL        0\nREFR        0\n", "SPECRGB     .9 .8 .7\nREFL        0.5\nREFR        0.5\n", 1)
    return head + sep + tail


_paths = {}


def scene_file(tmp_path_factory, depth, kind="cornell", eye=None):
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    key = (kind, depth, eye)
    if key not in _paths:
        text = _two_axes_text(depth) if kind == "two axes" else scenes.cornell_scene_text(depth=depth, eye=eye)
        _paths[key] = scenes.write_scene(text, str(tmp_path_factory.mktemp("primary_once") / f"{kind.replace(' ', '_')}_d{depth}{'_moved' if eye else ''}.txt"))
    return _paths[key]


def run(path, res, arith, flags, script, **kw):
    """What `script(renderer)` returns on a fresh renderer, and its statistics at the end."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(path, res=res), arith=arith, iters_per_batch=3, debug_flags=flags, **kw)
    try:
        out = script(r)
        return out, r.stats()
    finally:
        r.free()


def both_arms(path, res, arith, script, launches, flags=0, form=FIRST, **kw):
    """The outputs of `script` by default after asserting that the run with bit 65536 gives the same ones, the same samples and live
    rays; `launches`: PtStats.primary_launches (by default, with the bit)."""
    (out, st), (out_e, st_e) = (run(path, res, arith, flags | extra, script, **kw) for extra in (0, EVERY_BATCH))
    assert st.record_form == st_e.record_form == form
    assert (st.primary_launches, st_e.primary_launches) == launches
    assert len(out) == len(out_e)
    for i, (a, b) in enumerate(zip(out, out_e)):
        assert np.isfinite(a).all(), (arith, i)
        diff = (bits(a) != bits(b)).any(axis=1)
        assert not diff.any(), f"{arith}, output {i}: {diff.sum()} pixels differ from the run that traces depth 0 in every batch, first {np.flatnonzero(diff)[:8]}"
    assert st.samples == st_e.samples and list(st.live_rays) == list(st_e.live_rays)
    return out, st


_refs = {}


def reference(oracle, path, res, spp, depth, kw=None):
    key = (path, res, spp, tuple(sorted((kw or {}).items())))
    if key not in _refs:  # (computed once, read only)
        _refs[key] = _oracle_tile(oracle, path, res, spp, depth, kw or {})
    return _refs[key]


def ten(r):
    r.render(1, 10)
    return [r.readback()]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("res,depth", FRAMES, ids=FRAME_IDS)
@pytest.mark.parametrize("kind", ["cornell", "two axes"])
def test_ten_iterations_one_trace(tmp_path_factory, oracle, kind, res, depth, arith):
    path = scene_file(tmp_path_factory, depth, kind)
    (img,), st = both_arms(path, res, arith, ten, (1, 4))
    assert st.samples == res[0] * res[1] * 10 and st.live_rays[0] == st.samples and 0 < st.live_rays[1] < st.samples
    if arith == "exact":
        assert_is_oracle([img], reference(oracle, path, res, 10, depth))


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("res,depth", FRAMES, ids=FRAME_IDS)
def test_clear_keeps_the_first_hits_and_a_longer_batch_finds_its_counts(tmp_path_factory, oracle, res, depth, arith):
    path = scene_file(tmp_path_factory, depth)

    def cleared(r):  # batches of 3 and 1, then — the image zeroed, the records kept — 3, 3, 3 and 1
        r.render(1, 4)
        r.clear()
        return ten(r)

    def growing(r):  # the only trace belongs to a batch of 2; batches of 3 follow
        r.render(1, 2)
        r.render(3, 9)
        return [r.readback()]

    (img,), st = both_arms(path, res, arith, cleared, (1, 6))
    assert st.samples == res[0] * res[1] * 10  # (pt_clear zeroes the samples, not the launches)
    (img11,), _ = both_arms(path, res, arith, growing, (1, 4))
    if arith == "exact":
        assert_is_oracle([img], reference(oracle, path, res, 10, depth))
        assert_is_oracle([img11], reference(oracle, path, res, 11, depth))


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("res,depth", FRAMES, ids=FRAME_IDS)
def test_a_moved_camera_is_traced_again_once(tmp_path_factory, oracle, res, depth, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    here, there = scene_file(tmp_path_factory, depth), scene_file(tmp_path_factory, depth, eye=(0, 5, 30))
    seen = []

    def moved(r):
        first = ten(r)[0]
        seen.append(r.stats().primary_launches)
        r.set_camera(capi.Scene(there, res=res).camera)
        return [first] + ten(r)

    (first, second), _ = both_arms(here, res, arith, moved, (2, 8))
    assert seen == [1, 4]  # the launches before the move: it adds exactly one by default
    assert not np.array_equal(bits(first), bits(second))
    (fresh,), _ = run(there, res, arith, 0, ten)
    assert np.array_equal(bits(second), bits(fresh))
    if arith == "exact":
        assert_is_oracle([first], reference(oracle, here, res, 10, depth))
        assert_is_oracle([second], reference(oracle, there, res, 10, depth))


def _tiles(res):
    from cosc_4397_pathtracing_raytracing_project_amd import parallel
    begin, count = parallel.tile_for_rank(res[0], res[1], 1, 3)
    return [parallel.striped_tile_for_rank(res[0], res[1], 0, 8), dict(pixel_begin=begin, pixel_count=count)]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("res,depth", FRAMES, ids=FRAME_IDS)
@pytest.mark.parametrize("tile", [0, 1], ids=["rank 0 of 8, striped", "rank 1 of 3, contiguous"])
def test_a_rank_tile(tmp_path_factory, oracle, tile, res, depth, arith):
    path, kw = scene_file(tmp_path_factory, depth), _tiles(res)[tile]
    (img,), st = both_arms(path, res, arith, ten, (1, 4), **kw)
    assert st.samples == img.shape[0] * 10 and img.shape[0] < res[0] * res[1]
    if arith == "exact":
        assert_is_oracle([img], reference(oracle, path, res, 10, depth, kw))


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("res,depth", FRAMES, ids=FRAME_IDS)
def test_list_batches_between_uniform_ones(tmp_path_factory, oracle, res, depth, arith):
    """Two rounds over the noisiest quarter on the worker — its own records, traced once per round of two batches, for a list that
    is new behind the same pointer — between uniform batches of the renderer, whose records stay."""
    path = scene_file(tmp_path_factory, depth)

    def rounds(r):
        r.render(1, 3)
        r.noise_fold()
        r.render(4, 3)
        r.noise_fold()
        r.adaptive_round(7, 4, 0.25)
        r.adaptive_round(11, 4, 0.25)
        resolved, iterations = r.resolve(), r.readback_adaptive()[:, 0]
        assert iterations.min() == 6 and (iterations == 10).any()  # some pixel was in one list only: the two lists differ
        r.clear()  # back to the uniform state
        return [resolved] + ten(r)

    (_, img), st = both_arms(path, res, arith, rounds, (1, 6))
    if arith == "exact":
        assert_is_oracle([img], reference(oracle, path, res, 10, depth))


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("res,depth", FRAMES, ids=FRAME_IDS)
@pytest.mark.parametrize("name,flags,kw", [("aa_jitter", 0, dict(aa_jitter=True)), ("split records", SPLIT_RECORDS, {}), ("records by visit", BY_VISIT, {})],
                         ids=["aa_jitter", "8192", "16384"])
def test_other_forms_trace_in_every_batch(tmp_path_factory, name, flags, kw, res, depth, arith):
    path = scene_file(tmp_path_factory, depth)
    form = {"aa_jitter": 0, "split records": 1, "records by visit": FIRST}[name]
    (img,), _ = both_arms(path, res, arith, ten, (4, 4), flags=flags, form=form, **kw)
    if name != "aa_jitter":  # the same samples as the default form
        (plain,), _ = run(path, res, arith, 0, ten)
        assert np.array_equal(bits(img), bits(plain))
