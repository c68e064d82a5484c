"""The threshold selection's kernels (pt_stage_adaptive_select_threshold: key, radix select for rank cap, the count of pixels above,
the cut under the threshold, count, scan, scatter; csrc/pt_adaptive.hip) against the numpy restatement
tests/adaptive_threshold_ref.py: list, above and m, and no list entry written behind m (the Python wrapper checks that)."""
import numpy as np
import pytest

import adaptive_ref as ref
import adaptive_threshold_ref as tref
from adaptive_threshold_ref import caps, check

pytestmark = pytest.mark.gpu
SHAPES = ((1, 1), (64, 1), (97, 11), (97, 61))  # one pixel, a wave, 1067 pixels just past one 1024-pixel block, several blocks


@pytest.fixture(scope="module")
def renderer(scene_dir):
    """The stage entry points run on the default renderer's device and stream; its scene does not matter."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(16, 8)), iters_per_batch=1)
    yield capi
    r.free()


@pytest.mark.parametrize("name", ref.PATTERNS)
def test_device_selection_equals_restatement(renderer, name):
    capi = renderer
    seen = set()
    for W, R in SHAPES:
        planes, counts = ref.pattern(name, W, R)
        for case, threshold in tref.case_thresholds(planes[0, :, 3], W, R, counts).items():
            for cap in caps(W * R):
                above, m = check(capi.stage_adaptive_select_threshold, planes, counts, W, R, threshold, cap, (name, (W, R), case, cap))
                assert capi.adaptive_select_threshold_host(planes, counts, W, R, threshold, cap)[1:] == (above, m)
                seen.add((case, "capped" if above > cap else "empty" if m == 0 else "all"))
    assert {c for c, _ in seen} >= ({"zero", "past"} if name == "zero" else {"zero", "below", "past"})
    if name == "random":
        assert {"between"} <= {c for c, _ in seen} and {k for _, k in seen} == {"capped", "empty", "all"}


@pytest.mark.parametrize("name", ["three", "equal"])
def test_ties_at_the_threshold_are_refused_across_waves_and_blocks(renderer, name):
    capi = renderer
    for W, R in SHAPES:
        planes, counts, threshold = tref.tie_pattern(name, W, R)
        k = ref.keys(planes[0, :, 3], W, R, counts)
        ties = np.flatnonzero(k == tref.threshold_bits(threshold))
        if W * R > 1024:  # ties in more than one 64-pixel wave and more than one 1024-pixel block
            assert np.unique(ties // 64).size > 2 and np.unique(ties // 1024).size >= 2, (name, (W, R), ties.size)
        for cap in caps(W * R):
            above, m = check(capi.stage_adaptive_select_threshold, planes, counts, W, R, threshold, cap, (name, (W, R), cap))
            assert above == int((k > tref.threshold_bits(threshold)).sum())


def test_nan_is_above_on_the_device(renderer):
    capi = renderer
    W, R = 97, 11
    planes, counts = ref.pattern("random", W, R)
    planes[0, 1000, 3] = np.nan
    planes[0, 5, 3] = -np.nan
    for threshold, cap in ((1e18, W * R), (1e18, 4), (0.01, 15), (0.0, 300)):
        above, m = check(capi.stage_adaptive_select_threshold, planes, counts, W, R, threshold, cap, (threshold, cap))
        assert above >= 6 + 6  # both 3 x 3 neighbourhoods, cut to two rows by the tile's bottom and top edge


def test_stage_refuses_what_the_host_function_refuses(renderer):
    capi = renderer
    planes, counts = ref.pattern("random", 5, 1)
    for threshold in (-0.5, float("nan"), float("inf")):
        with pytest.raises(capi.PtError, match="threshold"):
            capi.stage_adaptive_select_threshold(planes, counts, 5, 1, threshold, 2)
