"""Where k_paths keeps its wave-uniform state (csrc/pt_kernels.hip cold_args / cold, pixel_of; DESIGN.md section 5, "What bounds it").

The LDS-table instances of the bounce kernel read their cold arguments again from the kernarg segment at the piece switch, in a gather
step and in the epilogue, form the piece plan again at the switch, and turn a tile pixel into a frame pixel by one add for a contiguous
tile and through the batch's fields, read where they are needed, for a striped tile or a pixel list.  None of that may change a sample,
a record, a slot or a counter.  A 96x64 cornell render at depth 8, nine iterations in batches of three — the first batch runs the plain
fixed-slot instance, the two behind it the instance that also gathers its predecessor — for every pixel-map form global_pixel has:
  exact      bit-equal to the oracle on the same pixels;
  fma, fast  bit-equal to the same render under PtOptions.debug_flags 131072 (result-neutral: every batch runs the plain instance and is
             gathered by a launch of its own), and within test_gpu_arith.py's bounds of the reference semantics.
The references are computed once per form and only read."""
import numpy as np
import pytest

from test_gpu_arith import check_tolerance
from test_gpu_first_hit_sharing import assert_is_oracle, bits
from test_gpu_primary_once import reference, scene_file

pytestmark = pytest.mark.gpu
EVERY_BATCH = 131072  # PtOptions.debug_flags: every batch gathered by a launch of its own
RES, DEPTH, K, ITERS = (96, 64), 8, 3, 9  # three batches of three
ARITHS = ["exact", "fma", "fast"]


def tiles():
    from cosc_4397_pathtracing_raytracing_project_amd import parallel
    w, h = RES
    return {
        "whole frame": {},
        "sub-tile": dict(pixel_begin=7 * w, pixel_count=31 * w),           # pixel_begin > 0; 2976 pixels: the last chunk holds 32
        "striped": parallel.striped_tile_for_rank(w, h, 1, 3),           # rows 1, 4, ..: a run of 96 out of every 288 from pixel 96
    }


def frame_pixels(kw):
    """Frame pixel index of every tile pixel, in tile order."""
    w, h = RES
    begin, count = kw.get("pixel_begin", 0), kw.get("pixel_count", 0) or w * h - kw.get("pixel_begin", 0)
    stripe, stride = kw.get("stripe_pixels", 0), kw.get("stripe_stride", 0)
    p = np.arange(count)
    return begin + p if not stripe else begin + p + (p // stripe) * (stride - stripe)


_libm = {}


def libm_frame(oracle, path):
    """The reference semantics' whole frame (LIBM math, the reference-literal loop): what fma and fast are held to."""
    if path not in _libm:
        oracle.set_math_mode(oracle.LIBM)
        oracle.load_scene(path, res=RES)
        _libm[path] = oracle.render(1, ITERS, depth=DEPTH, variant=oracle.LITERAL, nthreads=16).reshape(-1, 3)
    return _libm[path]


def render(path, arith, flags, script, **kw):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(path, res=RES), arith=arith, iters_per_batch=K, debug_flags=flags, **kw)
    try:
        out = script(r)
        return out, r.stats()
    finally:
        r.free()


def nine(r):
    r.render(1, ITERS)
    return r.readback()


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("form", ["whole frame", "sub-tile", "striped"])
def test_tile_forms(tmp_path_factory, oracle, form, arith):
    kw = tiles()[form]
    path = scene_file(tmp_path_factory, DEPTH)
    img, st = render(path, arith, 0, nine, **kw)
    assert st.inline_gathers == 2  # the plain instance ran once, the gathering instance twice
    assert np.isfinite(img).all() and img.shape[0] == frame_pixels(kw).size and st.samples == img.shape[0] * ITERS
    other, st_o = render(path, arith, EVERY_BATCH, nine, **kw)
    diff = (bits(img) != bits(other)).any(axis=1)
    assert st_o.inline_gathers == 0 and not diff.any(), f"{arith}, {form}: {diff.sum()} pixels differ from the plain instance's image, first {np.flatnonzero(diff)[:8]}"
    assert list(st.live_rays) == list(st_o.live_rays)
    if arith == "exact":
        assert_is_oracle([img], reference(oracle, path, RES, ITERS, DEPTH, kw))
    else:
        check_tolerance(img, libm_frame(oracle, path)[frame_pixels(kw)], ITERS, f"{arith} {form}")


@pytest.mark.parametrize("arith", ARITHS)
def test_pixel_list(tmp_path_factory, oracle, arith):
    """A list batch as the adaptive round issues it (the worker context, pt_stage_render_list): 1480 distinct frame pixels in no order,
    nine iterations in the worker's batches of three."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path = scene_file(tmp_path_factory, DEPTH)
    lst = np.random.default_rng(11).choice(RES[0] * RES[1], 1480, replace=False).astype(np.int32)

    def listed(r):
        r.render(1, ITERS)
        return r.readback(), capi.stage_render_list(lst, 1, ITERS)

    (plain, got), st = render(path, arith, 0, listed)
    # (PtStats counts the renderer's own batches: the frame render above.  The worker's counters are not exposed, so which instance its
    # list batches took is not asserted; both arms below and the frame's rows hold whichever it was.)
    assert st.inline_gathers == 2 and np.isfinite(got).all()
    (plain_o, other), _ = render(path, arith, EVERY_BATCH, listed)
    assert np.array_equal(bits(got), bits(other)) and np.array_equal(bits(plain), bits(plain_o))
    assert np.array_equal(bits(got), bits(plain[lst]))  # the listed rows of the frame
    if arith == "exact":
        assert_is_oracle([got], reference(oracle, path, RES, ITERS, DEPTH)[lst])
    else:
        check_tolerance(got, libm_frame(oracle, path)[lst], ITERS, f"{arith} pixel list")
