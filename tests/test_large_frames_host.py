"""What tests/test_gpu_large_frames.py relies on, checked on the CPU (no GPU): the inputs of tests/large_frames.py have the block, pass
and chunk counts they are named for; the reduce's inputs add up exactly in any order; and at the new frames the library's host
functions — the device tests' reference — equal the numpy restatements.  The host functions share their bodies with the kernels
(csrc/pt_adaptive.h, pt_group_select.h, pt_denoise.h), so a mistake in a shared header shows here."""
import math
import struct

import numpy as np
import pytest

import adaptive_ref
import adaptive_threshold_ref
import denoise_guided_ref
import denoise_ref
import group_select_ref
import large_frames as lf
from denoise_ref import bits, f32


@pytest.fixture(scope="module")
def capi():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    return capi


def dbits(x):
    return struct.pack("<d", x)


def same(got, want, what):
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(got.shape[0], -1).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:2]], want[bad[:2]])


# ---- 1. the reduce ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix, partials", lf.REDUCE_PIXELS)
def test_reduce_inputs_sum_exactly(capi, npix, partials):
    """Every estimate is an integer number of 2^-9 and the host's pixel-order sum is the exactly rounded sum: any order of the additions
    gives the same double, so the device's SSE can be held to the host's bit for bit."""
    assert lf.blocks(npix) == partials and -(-partials // lf.CHUNK) == {1024: 1, 1025: 2, 2050: 3}[partials]
    assert npix * 24 * 512 < 2 ** 53  # every partial sum of the estimates, in units of 2^-9, is an integer a double holds
    planes = lf.summable_planes(npix)
    w, sse = capi.history_noise_host(planes, lf.REDUCE_GROUPS, lf.REDUCE_ITERS, lf.REDUCE_SAMPLES)
    units = w.astype(np.float64) / lf.REDUCE_UNIT
    assert np.array_equal(units, np.rint(units)) and units.min() >= 0 and units.max() < 24 * 512
    q = planes[1, :, :3]
    same(w, ((q[:, 0] / f32(2) + q[:, 1] / f32(2)) + q[:, 2] / f32(2)).astype(f32), npix)
    assert dbits(sse) == dbits(lf.exact_sum(w)) == dbits(float(int(units.sum()) * lf.REDUCE_UNIT)) and sse > 0
    if npix == lf.REDUCE_PIXELS[-1][0]:
        for span in lf.SPIKE_SPANS:  # a partial that a wrong chunk index loses or doubles must be worth something
            s = lf.span_of(npix, span)
            assert s.stop - s.start == (5 if span == 2049 else 1024)
            _, part = capi.history_noise_host(planes[:, s], lf.REDUCE_GROUPS, lf.REDUCE_ITERS, lf.REDUCE_SAMPLES)
            assert part > 0 and dbits(part) == dbits(lf.exact_sum(w[s]))


def test_counted_form_sums_exactly(capi):
    """Counts of (2, 2) everywhere give the counted form the uniform form's divisors: W is the same plane, NE = 2, and the sum is exact."""
    npix = lf.REDUCE_PIXELS[1][0]
    planes = lf.summable_planes(npix)
    w, ne, _, sse = capi.history_noise_adaptive_host(planes, lf.uniform_counts(npix))
    want, want_sse = capi.history_noise_host(planes, lf.REDUCE_GROUPS, lf.REDUCE_ITERS, lf.REDUCE_SAMPLES)
    same(w, want, "W")
    assert (ne == f32(2)).all() and dbits(sse) == dbits(want_sse) == dbits(lf.exact_sum(w))


# ---- 2. the selection -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lf.SELECT_PATTERNS)
@pytest.mark.parametrize("W, R, groups", lf.SELECT_FRAMES, ids=lambda v: str(v))
def test_select_host_equals_restatement(capi, W, R, groups, name):
    n = W * R
    assert lf.blocks(n) == groups and -(-groups // lf.PASS) == {256: 1, 257: 2, 514: 3}[groups]
    planes, counts = adaptive_ref.pattern(name, W, R)
    m = n // 4
    got = capi.adaptive_select_host(planes, counts, W, R, m)
    assert np.array_equal(got, adaptive_ref.select(planes[0, :, 3], W, R, counts, m)), (W, R, name)
    if name == "equal":  # the ties run through every workgroup: the list is the first m pixels
        assert np.array_equal(got, np.arange(m))


def test_nan_and_threshold_hosts_equal_restatement(capi):
    W, R = lf.NAN_FRAME
    planes, counts = lf.nan_planes()
    assert sorted(p // lf.BLOCK // lf.PASS for p in lf.NAN_PIXELS) == [0, 1]
    for m in lf.NAN_LENGTHS:
        got = capi.adaptive_select_host(planes, counts, W, R, m)
        assert np.array_equal(got, adaptive_ref.select(planes[0, :, 3], W, R, counts, m)), m
    nan_keys = np.flatnonzero(adaptive_ref.keys(planes[0, :, 3], W, R, counts) == 0xFFFFFFFF)
    assert nan_keys.size == 12 and np.array_equal(capi.adaptive_select_host(planes, counts, W, R, 12), nan_keys)
    planes, counts, thresholds = lf.threshold_case("random", W, R)
    assert {"zero", "below", "between", "past"} <= set(thresholds)
    for name, thr in thresholds.items():
        adaptive_threshold_ref.check(capi.adaptive_select_threshold_host, planes, counts, W, R, thr, W * R // 4, name)


# ---- 3. the partition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", lf.PARTITION_PARTS)
def test_partition_host_equals_restatement(capi, n):
    seen = []
    for name, w, h, lst, groups in lf.partition_lists(n):
        assert lf.blocks(lst.size) == groups and groups >= lf.PASS, (name, lst.size)
        seen.append(groups)
        parts, counts = capi.group_partition_host(lst, w, h, n)
        want, want_counts = group_select_ref.partition(lst, w, n)
        assert int(counts.sum()) == lst.size and np.array_equal(counts, want_counts), (name, n, counts)
        row = lst.astype(np.int64) // w
        tiles = (row // n) * w + lst % w
        for i in range(n):
            assert np.array_equal(np.sort(parts[i]), np.sort(tiles[row % n == i])), (name, n, i)  # a permutation of the expected
            assert np.array_equal(parts[i], want[i]), (name, n, i)                                # ... in input order
        if name == "part 0 only":
            assert groups > lf.PASS and counts[0] == lst.size and not counts[1:].any()
    assert seen[:4] == [256, 257, 514, 264]


# ---- 4. the filter's levels -----------------------------------------------------------------------------------------------------------
def test_denoise_frame_has_the_groups_it_is_named_for():
    w, rows = lf.DENOISE_FRAME
    assert [lf.group_counts(rows, l) for l in range(4, 8)] == [9, 5, 3, 2] and rows - 8 * 64 == 9
    assert divmod(w, 64) == (2, 2)
    assert rows > 2 * 2 * 128  # a stencil of level 7 (rows y - 256 .. y + 256) lies inside the frame for y = 256 .. 264
    rgb, planes = lf.plain_inputs()
    hits, misses, zero_albedo = denoise_ref.frame_properties(rgb, planes)
    assert hits > 1000 and misses > 1000 and zero_albedo > 1000


@pytest.mark.parametrize("opts", lf.RESTATED_OPTIONS, ids=["default sigmas", "sigmas off"])
def test_denoise_host_equals_restatement(capi, opts):
    w, rows = lf.DENOISE_FRAME
    rgb, planes = lf.plain_inputs()
    same(capi.denoise_host(rgb, planes, w, rows, lf.DENOISE_SPP, **opts), denoise_ref.denoise(rgb, planes, w, rows, lf.DENOISE_SPP, **opts), opts)


@pytest.mark.parametrize("opts", lf.RESTATED_OPTIONS, ids=["default sigmas", "sigmas off"])
def test_denoise_guided_host_equals_restatement(capi, opts):
    w, rows = lf.DENOISE_FRAME
    rgb, planes, noise = lf.guided_inputs()
    nonpositive, zero_variance, decades = denoise_guided_ref.noise_properties(noise, lf.GUIDED_GROUPS, lf.GUIDED_ITERS)
    assert nonpositive > 0 and zero_variance > 0 and decades >= 6.0
    same(capi.denoise_guided_host(rgb, planes, noise, w, rows, lf.GUIDED_GROUPS, lf.GUIDED_ITERS, **opts),
         denoise_guided_ref.denoise_guided(rgb, planes, noise, w, rows, lf.GUIDED_GROUPS, lf.GUIDED_ITERS, **opts), opts)


def test_sigmas_off_makes_every_level_count(capi):
    """With the edge-stopping terms off, levels 7 and 8 differ in most pixels: the last level's taps reach the result."""
    w, rows = lf.DENOISE_FRAME
    rgb, planes = lf.plain_inputs()
    seven = capi.denoise_host(rgb, planes, w, rows, lf.DENOISE_SPP, levels=7, **lf.OFF)
    eight = capi.denoise_host(rgb, planes, w, rows, lf.DENOISE_SPP, levels=8, **lf.OFF)
    assert (bits(seven) != bits(eight)).any(axis=1).mean() > 0.9


def test_sse_bound_reasoning():
    """(n - 1) 2^-53 at the renderer case's frame against the suite's relative 1e-9."""
    n = lf.RENDER_RES[0] * lf.RENDER_RES[1]
    assert lf.blocks(n) == 1025 and (n - 1) * 2.0 ** -53 * 8 < lf.SSE_RTOL and math.ceil(lf.RENDER_FRACTION * n) == 16400
