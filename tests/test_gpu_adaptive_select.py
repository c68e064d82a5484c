"""The selection's kernels (pt_stage_adaptive_select: key, radix select, count, scan, scatter; csrc/pt_adaptive.hip) against the
host function on the shapes, list lengths and estimate patterns of tests/adaptive_ref.py.  The list must be identical, so its
ascending order and the tie rule are checked too; the host function is pinned to the restatement by test_adaptive_host.py."""
import numpy as np
import pytest

import adaptive_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer(scene_dir):
    """The stage entry points run on the default renderer's device and stream; its scene does not matter."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(16, 8)), iters_per_batch=1)
    yield capi
    r.free()


@pytest.mark.parametrize("name", ref.PATTERNS)
def test_device_list_equals_host_list(renderer, name):
    capi = renderer
    for W, R in ref.SHAPES:
        planes, counts = ref.pattern(name, W, R)
        for m in ref.list_lengths(W * R):
            want = capi.adaptive_select_host(planes, counts, W, R, m)
            got = capi.stage_adaptive_select(planes, counts, W, R, m)
            assert np.array_equal(got, want), (name, (W, R), m, np.flatnonzero(got != want)[:8], got[:8], want[:8])


def test_nan_sorts_first_on_the_device(renderer):
    capi = renderer
    W, R = 97, 11
    planes, counts = ref.pattern("random", W, R)
    planes[0, 1000, 3] = np.nan
    planes[0, 5, 3] = -np.nan
    for m in (1, 15, 300):
        assert np.array_equal(capi.stage_adaptive_select(planes, counts, W, R, m), capi.adaptive_select_host(planes, counts, W, R, m)), m
