"""The stream gather of a batch inside the next batch's k_paths (csrc/pt_sched.h inline_gather).

A stream-gathered batch that another batch of the same pt_render call follows leaves its gather to that batch's bounce kernel, whose
waves add its records to the image beside their own work; the two batches store their records in different planes, and the last batch
of a call is gathered by k_collect_stream as before.  Which launch adds a batch's records changes no sample and no order of summation:
image, live-ray counts and sample count must be, bit for bit and in exact, fma and fast, those of PtOptions.debug_flags 131072, which
gathers every batch by a launch of its own (the code as it was), and in exact mode the oracle's image.  PtStats.inline_gathers counts
the batches that were gathered inside a bounce kernel, so every case also says how many it expects.

All frames are small and iters_per_batch is forced small, so that a call spans several batches.  Every render runs on a FRESH context:
both record planes start as NaN colours, so a slot gathered from the wrong plane shows."""
import numpy as np
import pytest

from test_gpu_first_hit_sharing import assert_is_oracle, bits
from test_gpu_primary_once import reference, scene_file

pytestmark = pytest.mark.gpu
EVERY_BATCH = 131072                     # PtOptions.debug_flags: every batch gathered by a launch of its own
TILE_FIXED, STREAM = 1, 2                # PtStats.gather_form after a render call
ARITHS = ["exact", "fma", "fast"]


def run(path, res, arith, flags, script, **kw):
    """What `script(renderer)` returns on a fresh renderer, and its statistics at the end."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(path, res=res), arith=arith, debug_flags=flags, **kw)
    try:
        out = script(r)
        return out, r.stats()
    finally:
        r.free()


def both_arms(path, res, arith, script, inline, form=STREAM, **kw):
    """The outputs of `script` by default, after asserting that the run with bit 131072 gives the same ones, the same samples and the
    same live rays; `inline`: PtStats.inline_gathers by default (with the bit: none)."""
    (out, st), (out_e, st_e) = (run(path, res, arith, flags, script, **kw) for flags in (0, EVERY_BATCH))
    assert (st.inline_gathers, st_e.inline_gathers) == (inline, 0)
    assert st.gather_form == st_e.gather_form == form  # nothing waits when a call has returned
    assert len(out) == len(out_e)
    for i, (a, b) in enumerate(zip(out, out_e)):
        assert np.isfinite(a).all(), f"{arith}, output {i}: {(~np.isfinite(a)).any(axis=1).sum()} pixels are not finite"
        diff = (bits(a) != bits(b)).any(axis=1)
        assert not diff.any(), f"{arith}, output {i}: {diff.sum()} pixels differ from the run that gathers every batch on its own, first {np.flatnonzero(diff)[:8]}"
    assert st.samples == st_e.samples and list(st.live_rays) == list(st_e.live_rays)
    return out, st


def steps(n):
    def script(r):
        r.render(1, n)
        return [r.readback()]
    return script


# (id, resolution, trace depth, iterations per batch, iterations, batches gathered inside the next one, tile)
CASES = [
    ("batches of 4, 4, 4 and 1", (96, 64), 8, 4, 13, 3, {}),       # the last K differs
    ("two batches", (96, 64), 8, 4, 8, 1, {}),                    # one gather inside k_paths, one on its own
    ("one batch", (96, 64), 8, 4, 4, 0, {}),                      # nothing to leave to anybody
    ("one iteration per batch", (96, 64), 8, 1, 3, 2, {}),
    ("gap slots", (97, 61), 8, 3, 7, 2, {}),                      # 5917 pixels: the tile's last chunk has 29
    ("depth 2", (64, 48), 2, 3, 10, 3, {}),                       # every path dies in the round after it was taken
]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name,res,depth,k,iters,inline,kw", CASES, ids=[c[0] for c in CASES])
def test_same_image_as_a_gather_per_batch(tmp_path_factory, oracle, name, res, depth, k, iters, inline, kw, arith):
    path = scene_file(tmp_path_factory, depth)
    (img,), st = both_arms(path, res, arith, steps(iters), inline, iters_per_batch=k, **kw)
    assert st.samples == img.shape[0] * iters and 0 < st.live_rays[1] < st.samples  # survivor slots and retiree slots exist
    if arith == "exact":
        assert_is_oracle([img], reference(oracle, path, res, iters, depth, kw))


@pytest.mark.parametrize("arith", ARITHS)
def test_fewer_slot_groups_than_waves(tmp_path_factory, oracle, arith):
    """Rank 0's striped tile of eight at 160x90: 1800 pixels, 29 chunks — most waves of a queue have no group to gather and the
    queues behind the 29th own no pixel at all."""
    from cosc_4397_pathtracing_raytracing_project_amd import parallel
    res, depth, kw = (160, 90), 8, parallel.striped_tile_for_rank(160, 90, 0, 8)
    path = scene_file(tmp_path_factory, depth)
    (img,), st = both_arms(path, res, arith, steps(10), 2, iters_per_batch=4, **kw)  # batches of 4, 4 and 2
    assert img.shape[0] < res[0] * res[1] // 7 and st.num_queues * 64 > img.shape[0]  # some queues are empty
    if arith == "exact":
        assert_is_oracle([img], reference(oracle, path, res, 10, depth, kw))


@pytest.mark.parametrize("arith", ARITHS)
def test_render_calls_back_to_back_and_a_clear_between(tmp_path_factory, oracle, arith):
    """Nothing waits across calls: the second call starts from a gathered image in whichever plane the first one ended, and pt_clear
    between two calls zeroes a complete image."""
    res, depth = (96, 64), 8
    path = scene_file(tmp_path_factory, depth)

    def two_calls(r):  # batches of 4, 4, 3, then 4, 2
        r.render(1, 11)
        first = r.readback()
        r.render(12, 6)
        return [first, r.readback()]

    def cleared(r):  # batches of 4, 3, then — the image zeroed — 4, 4, 4, 1
        r.render(1, 7)
        r.clear()
        r.render(1, 13)
        return [r.readback()]

    (first, img17), _ = both_arms(path, res, arith, two_calls, 3, iters_per_batch=4)
    (img13,), st = both_arms(path, res, arith, cleared, 4, iters_per_batch=4)
    assert st.samples == res[0] * res[1] * 13
    if arith == "exact":
        assert_is_oracle([first], reference(oracle, path, res, 11, depth))
        assert_is_oracle([img17], reference(oracle, path, res, 17, depth))
        assert_is_oracle([img13], reference(oracle, path, res, 13, depth))


@pytest.mark.parametrize("arith", ARITHS)
def test_a_moved_camera_between_calls(tmp_path_factory, oracle, arith):
    """The first batch after pt_set_camera traces depth 0 again into plane 0 and gathers nobody; the batches behind it go on as before."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res, depth = (96, 64), 8
    here, there = scene_file(tmp_path_factory, depth), scene_file(tmp_path_factory, depth, eye=(0, 5, 30))

    def moved(r):  # batches of 4, 4, 2 for either camera
        r.render(1, 10)
        first = r.readback()
        r.set_camera(capi.Scene(there, res=res).camera)
        r.render(1, 10)
        return [first, r.readback()]

    (first, second), st = both_arms(here, res, arith, moved, 4, iters_per_batch=4)
    assert st.primary_launches == 2 and not np.array_equal(bits(first), bits(second))
    if arith == "exact":
        assert_is_oracle([first], reference(oracle, here, res, 10, depth))
        assert_is_oracle([second], reference(oracle, there, res, 10, depth))


@pytest.mark.parametrize("arith", ARITHS)
def test_the_convergence_metric_keeps_a_gather_per_batch(scene_dir, arith):
    """A context with the metric gathers every batch by a launch of its own — the stream before the reference frame is captured, the
    tile gather from then on — and its curve and image are those of the switch."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res, iters = (97, 61), 12

    def run_metric(flags):
        r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=res), convergence=7, iters_per_batch=3, arith=arith, debug_flags=flags)
        try:
            r.render(1, 6)  # two batches before the capture
            early = (r.stats().gather_form, r.stats().inline_gathers)
            r.render(7, iters - 6)
            return r.convergence(1, iters), r.readback(), early, (r.stats().gather_form, r.stats().inline_gathers)
        finally:
            r.free()

    sse, img, early, late = run_metric(0)
    sse_e, img_e, early_e, late_e = run_metric(EVERY_BATCH)
    assert early == early_e == (STREAM, 0) and late == late_e == (TILE_FIXED, 0)
    assert np.isfinite(img).all() and np.array_equal(bits(img), bits(img_e))
    assert np.array_equal(sse.view(np.uint64), sse_e.view(np.uint64)) and (sse[7:] > 0).all()
