"""The pixel-list form of the path-tracing kernels (BatchInfo::list, csrc/pt_kernels.hip global_pixel) through the worker context
alone (pt_stage_render_list): the group sum of a list equals, bit for bit, the listed rows of a plain renderer's image of the same
iterations — whatever the list's order and length, the arithmetic mode, the kernel forms and the search form."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RES = (97, 61)
ITERS = 7  # with iters_per_batch = 3: two full batches and a cut one
LENGTHS = (1, 50, 64, 65, 1480)
_PLAIN = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lists(n, seed=5):
    """Random distinct tile pixels for every length, sorted and shuffled."""
    rng = np.random.default_rng(seed)
    for m in LENGTHS:
        pick = rng.choice(n, m, replace=False).astype(np.int32)
        yield m, "shuffled", pick
        yield m, "sorted", np.sort(pick)


def check(path, res, **kw):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(path, res=res), iters_per_batch=3, **kw)
    try:
        before = r.stats().device_bytes
        r.render(1, ITERS)
        plain = r.readback()
        assert np.isfinite(plain).all() and plain.max() > 0
        for m, order, lst in lists(plain.shape[0]):
            got = capi.stage_render_list(lst, 1, ITERS)
            bad = np.flatnonzero((bits(got) != bits(plain[lst])).any(axis=1))
            assert bad.size == 0, (kw, m, order, bad.size, lst[bad[:4]], got[bad[:2]], plain[lst[bad[:2]]])
        assert np.array_equal(bits(r.readback()), bits(plain))  # the renderer's own image is untouched
        assert r.stats().device_bytes > before                  # the worker's memory is accounted for
    finally:
        r.free()


@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
@pytest.mark.parametrize("aa_jitter", [True, False], ids=["jitter", "shared"])
def test_list_equals_rows_of_the_plain_image(scene_dir, arith, aa_jitter):
    # without jitter the worker runs the shared first-hit form, retire_once and split_records
    check(scene_dir["cornell"], RES, arith=arith, aa_jitter=aa_jitter)


def test_unfused_kernels(scene_dir):
    check(scene_dir["cornell"], RES, aa_jitter=True, unfused_primary=True, unfused_bounces=True)


@pytest.mark.parametrize("aa_jitter", [True, False], ids=["jitter", "shared"])
def test_scan_form(scene_dir, aa_jitter):
    check(scene_dir["stress"], RES, aa_jitter=aa_jitter)


@pytest.mark.parametrize("aa_jitter", [True, False], ids=["jitter", "shared"])
def test_grid_walk(scene_dir, aa_jitter):
    check(scene_dir["stress_big"], RES, aa_jitter=aa_jitter, debug_flags=256)


def test_refusals(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(33, 9)), iters_per_batch=3)
    try:
        before = r.stats().device_bytes
        for lst in ([0, 0], [0, 33 * 9], [-1]):
            with pytest.raises(capi.PtError, match="outside the tile or repeated"):
                capi.stage_render_list(np.array(lst, np.int32), 1, 1)
        with pytest.raises(capi.PtError, match="bad argument"):
            capi.stage_render_list(np.array([1], np.int32), 0, 1)
        assert r.stats().device_bytes == before
    finally:
        r.free()
