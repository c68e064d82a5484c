"""Adaptive sampling's selection by threshold on the host (pt_adaptive_select_threshold_host; no GPU) against the numpy restatement
tests/adaptive_threshold_ref.py: list, above and m."""
import numpy as np
import pytest

import adaptive_ref as ref
import adaptive_threshold_ref as tref
from adaptive_threshold_ref import caps, check


@pytest.fixture(scope="module")
def capi():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    return capi


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ref.PATTERNS)
def test_select_threshold_host_equals_restatement(capi, shape, name):
    W, R = shape
    n = W * R
    planes, counts = ref.pattern(name, W, R)
    thresholds = tref.case_thresholds(planes[0, :, 3], W, R, counts)
    assert {"zero", "past"} <= set(thresholds) and (name == "zero" or n == 1 or "below" in thresholds), (shape, name, thresholds)
    for case, threshold in thresholds.items():
        for cap in caps(n):
            above, m = check(capi.adaptive_select_threshold_host, planes, counts, W, R, threshold, cap, (shape, name, case, cap))
            if case == "past":
                assert (above, m) == (0, 0)
            if case in ("zero", "below"):  # every pixel with a non-zero key; a zero-variance pixel is never above
                k = ref.keys(planes[0, :, 3], W, R, counts)
                assert above == int((k != 0).sum())


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["three", "equal"])
def test_a_key_equal_to_the_threshold_is_not_above(capi, shape, name):
    W, R = shape
    n = W * R
    planes, counts, threshold = tref.tie_pattern(name, W, R)
    k = ref.keys(planes[0, :, 3], W, R, counts)
    thr = tref.threshold_bits(threshold)
    ties = int((k == thr).sum())
    assert ties == n if name == "equal" else ties > 0 or W < 10, (shape, name, ties)  # (a tile narrower than two bands has the first band only)
    for cap in caps(n):
        above, m = check(capi.adaptive_select_threshold_host, planes, counts, W, R, threshold, cap, (shape, name, cap))
        assert above == int((k > thr).sum()) <= n - ties
    if name == "three" and n > 1000:
        # the bands exist at this size (of a band's 5 columns the inner 3 carry its value exactly): more refused ties than a wave
        # holds, and pixels above as well as below beside them
        assert ties > 128 and 128 < above < n - ties - 128


def test_between_two_keys_and_a_nan_estimate(capi):
    W, R = 97, 11
    planes, counts = ref.pattern("random", W, R)
    thresholds = tref.case_thresholds(planes[0, :, 3], W, R, counts)
    assert "between" in thresholds
    above, m = check(capi.adaptive_select_threshold_host, planes, counts, W, R, thresholds["between"], W * R, "between")
    assert 0 < above < W * R
    planes[0, 500, 3] = np.nan  # poisons the keys of its 3x3 neighbourhood: all nine are above whatever the threshold
    y, x = divmod(500, W)
    nine = np.sort([(y + j) * W + x + i for j in (-1, 0, 1) for i in (-1, 0, 1)])
    got, above, m = capi.adaptive_select_threshold_host(planes, counts, W, R, 1e18, W * R)
    assert (above, m) == (9, 9) and np.array_equal(got, nine)
    got, above, m = capi.adaptive_select_threshold_host(planes, counts, W, R, thresholds["between"], 9)  # ... and sort first under a cap
    assert above > 9 and m == 9 and np.array_equal(got, nine)
    check(capi.adaptive_select_threshold_host, planes, counts, W, R, thresholds["between"], 9, "nan under a cap")


def test_select_threshold_host_refuses(capi):
    import ctypes as C
    planes, counts = ref.pattern("random", 5, 1)
    for threshold in (-0.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(capi.PtError, match="threshold"):
            capi.adaptive_select_threshold_host(planes, counts, 5, 1, threshold, 2)
    z, c = np.ascontiguousarray(planes).reshape(-1), np.ascontiguousarray(counts).reshape(-1)
    out, above, m = np.full(8, -1, np.int32), C.c_int32(-1), C.c_int32(-1)
    for cap in (0, 6, -1):  # (the C function itself; the Python wrapper refuses these before it is called)
        assert capi.lib().pt_adaptive_select_threshold_host(5, 1, capi._f(z), capi._i(c), C.c_float(0.1), cap, capi._i(out), C.byref(above), C.byref(m)) != 0
        assert b"a list of" in capi.lib().pt_last_error() and (out == -1).all() and (above.value, m.value) == (-1, -1)
        with pytest.raises(capi.PtError):
            capi.adaptive_select_threshold_host(planes, counts, 5, 1, 0.1, cap)
    counts[3, 0] = 0
    with pytest.raises(capi.PtError, match="no iterations"):
        capi.adaptive_select_threshold_host(planes, counts, 5, 1, 0.1, 2)
