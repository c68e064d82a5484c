"""The post-processing kernels at frames past one reduce chunk, one scan pass and one row group of the filter's upper levels
(tests/large_frames.py names the thresholds), against the library's host functions, bit for bit.  The host functions are pinned to the
numpy restatements at these frames by tests/test_large_frames_host.py, which also checks that every input has the block, pass and chunk
count it is named for.  Everything but the last test goes through the stage entry points on a small live renderer."""
import struct

import numpy as np
import pytest

import adaptive_ref
import large_frames as lf
import noise_ref
from denoise_ref import bits, f32

pytestmark = pytest.mark.gpu


@pytest.fixture()
def capi(scene_dir):
    """The stage entry points run on the default renderer's device and stream; its scene does not matter."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(16, 8)), iters_per_batch=1)
    yield capi
    r.free()


@pytest.fixture(scope="module")
def largest():
    """The dense planes of the largest reduce size (67 MB), the host's W and SSE of them, and a zeroed buffer for the spike cases."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    npix = lf.REDUCE_PIXELS[-1][0]
    planes = lf.summable_planes(npix)
    w, sse = capi.history_noise_host(planes, lf.REDUCE_GROUPS, lf.REDUCE_ITERS, lf.REDUCE_SAMPLES)
    return planes, w, sse, np.zeros_like(planes)


def dbits(x):
    return struct.pack("<d", x)


def same(got, want, what):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


def estimate(capi, planes):
    return capi.stage_history_noise(planes, lf.REDUCE_GROUPS, lf.REDUCE_ITERS, lf.REDUCE_SAMPLES)


# ---- 1. the reduce over more than one chunk ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix, partials", lf.REDUCE_PIXELS)
def test_reduce_dense_sum_equals_host_bit_for_bit(capi, largest, npix, partials):
    """The estimates add up exactly in any order (test_large_frames_host.py), so the double that leaves k_noise_reduce must be the
    host's, bit for bit: a partial lost, doubled or read from the wrong chunk changes it."""
    if npix == largest[0].shape[1]:
        planes, want_w, want_sse, _ = largest
    else:
        planes = lf.summable_planes(npix)
        want_w, want_sse = capi.history_noise_host(planes, lf.REDUCE_GROUPS, lf.REDUCE_ITERS, lf.REDUCE_SAMPLES)
    w, sse = estimate(capi, planes)
    same(w, want_w, (npix, "W"))
    assert dbits(sse) == dbits(want_sse), (npix, partials, sse, want_sse, (sse - want_sse) / lf.REDUCE_UNIT)


@pytest.mark.parametrize("span", lf.SPIKE_SPANS)
def test_reduce_keeps_every_partial(capi, largest, span):
    """q is zero except in one span of 1,024 pixels (the last span: five), at the largest size: the SSE is that span's own sum, which
    names the partial that a wrong chunk index loses or doubles."""
    dense, dense_w, _, planes = largest
    npix = dense.shape[1]
    s = lf.span_of(npix, span)
    planes[1, s] = dense[1, s]
    try:
        _, want_sse = capi.history_noise_host(dense[:, s], lf.REDUCE_GROUPS, lf.REDUCE_ITERS, lf.REDUCE_SAMPLES)
        w, sse = estimate(capi, planes)
    finally:
        planes[1, s] = 0
    want_w = np.zeros(npix, f32)
    want_w[s] = dense_w[s]
    same(w, want_w, (span, "W"))
    assert want_sse > 0 and dbits(sse) == dbits(want_sse), (span, sse, want_sse)


def test_reduce_counted_form_equals_host_bit_for_bit(capi):
    """pt_history_threshold.hip's pass A feeds the same reduce.  Counts of (2, 2) in every pixel keep the divisors powers of two, so the
    counted form's estimates are the uniform form's and add up exactly: W, NE and the SSE are the host's bit for bit."""
    npix = lf.REDUCE_PIXELS[1][0]
    planes, counts = lf.summable_planes(npix), lf.uniform_counts(npix)
    w, ne, sse = capi.stage_history_noise_adaptive(planes, counts)
    want_w, want_ne, _, want_sse = capi.history_noise_adaptive_host(planes, counts)
    same(w, want_w, "W"), same(ne, want_ne, "NE")
    assert dbits(sse) == dbits(want_sse), (sse, want_sse)


# ---- 2. selection with more than one scan pass ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lf.SELECT_PATTERNS)
@pytest.mark.parametrize("W, R, groups", lf.SELECT_FRAMES, ids=lambda v: str(v))
def test_select_list_equals_host_list(capi, W, R, groups, name):
    """A wrong carry between the passes of k_adaptive_scan moves every entry behind the first 256 workgroups; `equal` with m = n - 1
    and m = n runs the ties through every pass."""
    planes, counts = adaptive_ref.pattern(name, W, R)
    for m in adaptive_ref.list_lengths(W * R):
        want = capi.adaptive_select_host(planes, counts, W, R, m)
        got = capi.stage_adaptive_select(planes, counts, W, R, m)
        assert np.array_equal(got, want), (name, (W, R), m, np.flatnonzero(got != want)[:8], got[:8], want[:8])


def test_select_nan_in_each_pass_sorts_first(capi):
    W, R = lf.NAN_FRAME
    planes, counts = lf.nan_planes()
    for m in lf.NAN_LENGTHS:
        assert np.array_equal(capi.stage_adaptive_select(planes, counts, W, R, m), capi.adaptive_select_host(planes, counts, W, R, m)), m


@pytest.mark.parametrize("name", lf.THRESHOLD_PATTERNS)
@pytest.mark.parametrize("W, R, groups", lf.THRESHOLD_FRAMES, ids=lambda v: str(v))
def test_select_by_threshold_equals_host(capi, W, R, groups, name):
    planes, counts, thresholds = lf.threshold_case(name, W, R)
    for what, thr in thresholds.items():
        for cap in lf.threshold_caps(W * R):
            got = capi.stage_adaptive_select_threshold(planes, counts, W, R, thr, cap)
            want = capi.adaptive_select_threshold_host(planes, counts, W, R, thr, cap)
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (name, (W, R), what, cap, got[1:], want[1:])


def test_history_selections_equal_host(capi):
    """The selection by threshold over the blend's keys and the history round's selection, each once at 513 x 512: both run the
    selection's count, scan and scatter on keys of their own."""
    W, R, _ = lf.SELECT_FRAMES[1]
    noise, counts, Cp, VC, thr, cap = lf.blend_select_case(W, R)
    got = capi.stage_history_select_threshold_blend(noise, counts, W, R, thr, cap, Cp, VC)
    want = capi.history_select_threshold_blend_host(noise, counts, W, R, thr, cap, Cp, VC)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:] and want[2] > lf.PASS * lf.BLOCK // 8, (got[1:], want[1:])
    feat, Cp, emitter = lf.history_select_case(W, R)
    got, got_fresh, got_m = capi.stage_history_select(feat, W, R, Cp, emitter)
    want, want_fresh, want_m = capi.history_select_host(feat, W, R, Cp, emitter)
    assert (got_fresh, got_m) == (want_fresh, want_m) and want_m > 1000, (got_fresh, got_m, want_fresh, want_m)
    assert np.array_equal(got, want) and got[want_m - 1] >= lf.PASS * lf.BLOCK  # (the entries behind m are -1 on both sides)


# ---- 3. partition with more than one scan pass ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", lf.PARTITION_PARTS)
def test_partition_equals_host(capi, n):
    """A wrong carry in k_partition_scan moves a part's entries behind its first 256 workgroups; `part 0 only` leaves every other part
    with zero counts in every workgroup of every pass."""
    for name, w, h, lst, _ in lf.partition_lists(n):
        want_parts, want_counts = capi.group_partition_host(lst, w, h, n)
        parts, counts = capi.stage_group_partition(lst, w, h, n)
        assert np.array_equal(counts, want_counts), (n, name, counts, want_counts)
        for i in range(n):
            assert np.array_equal(parts[i], want_parts[i]), (n, name, i, np.flatnonzero(parts[i] != want_parts[i])[:8], parts[i][:8], want_parts[i][:8])


# ---- 4. à-trous levels with several row groups and more than two x tiles ----------------------------------------------------------------
def test_denoise_equals_host(capi):
    w, rows = lf.DENOISE_FRAME
    rgb, planes = lf.plain_inputs()
    for opts in lf.PLAIN_OPTIONS:
        same(capi.Renderer.stage_denoise(rgb, planes, w, rows, lf.DENOISE_SPP, **opts), capi.denoise_host(rgb, planes, w, rows, lf.DENOISE_SPP, **opts), opts)


def test_denoise_guided_and_adaptive_equal_host(capi):
    w, rows = lf.DENOISE_FRAME
    rgb, planes, noise, counts = lf.adaptive_inputs()
    M, T = lf.GUIDED_GROUPS, lf.GUIDED_ITERS
    for opts in lf.RESTATED_OPTIONS:
        same(capi.Renderer.stage_denoise_guided(rgb, planes, noise, w, rows, M, T, **opts), capi.denoise_guided_host(rgb, planes, noise, w, rows, M, T, **opts),
             ("guided", opts))
        same(capi.Renderer.stage_denoise_adaptive(rgb, planes, noise, counts, w, rows, **opts),
             capi.denoise_adaptive_host(rgb, planes, noise, counts, w, rows, **opts), ("adaptive", opts))


def test_history_denoise_moments_equals_host(capi):
    w, rows = lf.DENOISE_FRAME
    S, planes, Cp, VC = lf.moments_inputs()
    for opts in lf.RESTATED_OPTIONS:
        same(capi.stage_history_denoise_moments(S, planes, w, rows, lf.MOMENTS_SPP, Cp, VC, **opts),
             capi.history_denoise_moments_host(S, planes, w, rows, lf.MOMENTS_SPP, Cp, VC, **opts), opts)


# ---- 5. one renderer case at a frame with more than 1,024 partials ----------------------------------------------------------------------
def raw_planes(r, capi):
    out = np.empty((2, r.n, 4), f32)
    capi._check(capi.lib().pt_readback_noise(capi._f(out)))
    return out


def test_renderer_folds_and_one_round_at_1025_partials(scene_dir):
    """test_gpu_adaptive.py's rounds against the restatement, cut down to two folds and one round, on cornell at 1025 x 1024: the fold's
    SSE and the merge's (k_adaptive_partial) both pass through the reduce's second chunk, and the round's selection through the five
    passes of the scan over 1,025 workgroups.  The SSEs are held to the suite's relative 1e-9 of math.fsum of the restated estimates: summing n non-negative doubles
    in any order stays within (n - 1) 2^-53 = 1.2e-10 of the exact sum at this n."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    W, R = lf.RENDER_RES
    N = W * R
    scene = capi.Scene(scene_dir["cornell"], res=lf.RENDER_RES)
    plain = capi.Renderer(scene, iters_per_batch=1)
    try:
        plain.render(3, 1)  # a worker's group sum starts at zero: the round's is this image
        group_sum = plain.readback()
    finally:
        plain.free()
    r = capi.Renderer(scene, iters_per_batch=1)
    try:
        planes = noise_ref.new_planes(N)
        for M in (1, 2):
            r.render(M, 1)
            r.noise_fold()
            S = r.readback()
            noise_ref.fold(S, planes, 1, M, M)
        same(raw_planes(r, capi), planes, "planes after two folds")
        noise, exact = r.noise(), lf.exact_sum(planes[0, :, 3])
        print(f"fold: sse {noise['sse']!r} exact {exact!r} relative {(noise['sse'] - exact) / exact:.3e}")
        assert (noise["groups"], noise["iterations"]) == (2, 2)
        assert exact > 0 and abs(noise["sse"] - exact) <= lf.SSE_RTOL * exact, (noise["sse"], exact)

        counts = adaptive_ref.uniform_counts(N, 2, 2)
        assert np.array_equal(r.readback_adaptive(), counts)
        m = adaptive_ref.list_length(lf.RENDER_FRACTION, N)
        lst = adaptive_ref.select(planes[0, :, 3], W, R, counts, m)
        assert lst[0] < lf.PASS * lf.BLOCK <= lst[-1]  # the list has entries in the scan's first pass and behind it
        adaptive_ref.merge(S, planes, counts, lst, group_sum[lst], 1)
        r.adaptive_round(3, 1, lf.RENDER_FRACTION)
        assert np.array_equal(r.readback_adaptive(), counts)
        same(r.readback(), S, "SUM image after the round"), same(raw_planes(r, capi), planes, "planes after the round")
        same(r.resolve(), adaptive_ref.resolve(S, counts), "resolve")
        noise, exact = r.noise(), lf.exact_sum(planes[0, :, 3])
        print(f"merge: sse {noise['sse']!r} exact {exact!r} relative {(noise['sse'] - exact) / exact:.3e}")
        assert (noise["groups"], noise["iterations"]) == (3, 3)
        assert exact > 0 and abs(noise["sse"] - exact) <= lf.SSE_RTOL * exact, (noise["sse"], exact)
        assert r.stats().samples == 2 * N + m
    finally:
        r.free()
