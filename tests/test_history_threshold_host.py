"""Threshold rounds over the blend on the host (the pt_history_*_adaptive_host twins and pt_history_select_threshold_blend_host:
csrc/pt_history.h and csrc/pt_denoise.h, the bodies the HIP kernels run too) against the numpy restatement
tests/history_threshold_ref.py, bit for bit, and the identities that tie them to the calls the library had before.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import adaptive_ref
import denoise_ref
import history_threshold_ref as ref
from history_ref import bits, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "csrc")
SHAPE_IDS = [f"{w}x{r}" for w, r in ref.SHAPES]


def same(got, want, what=""):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


def same_double(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b)


def inputs(W, R):
    """counts, the planes a render could have left, its SUM image, made-up feature planes and C, VC of one shape."""
    n = W * R
    counts = ref.random_counts(n)
    noise, S = ref.noise_planes(counts)
    _, feat = denoise_ref.random_frame(W, R, 4)
    C, VC = ref.current_planes(n, 3 * n)
    return counts, noise, S, feat, C, VC


def tame(VC):
    """VC for the filter: the restatement multiplies a skipped tap's variance by a weight of 0 where the library skips the tap, which
    differs for a NaN or an infinity (0 * inf); the huge variances overflow once demodulated, so they go too."""
    return np.where(np.isfinite(VC) & (VC < f32(1e30)), VC, f32(2.0)).astype(f32)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=SHAPE_IDS)
def test_pass_a_blend_and_capture_equal_the_restatement(shape):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    W, R = shape
    counts, noise, S, feat, C, VC = inputs(W, R)
    assert counts[:, 0].min() == 2 and counts[:, 0].max() == 40 or W * R < 100
    for cur, var, what in ((None, None, "absent"), (C, VC, "present")):
        w, ne, vb, sse = capi.history_noise_adaptive_host(noise, counts, cur, var)
        want_w, want_ne, want_vb, want_sse = ref.noise_counts(noise, counts, cur, var)
        same(w, want_w, f"W {shape} {what}"), same(ne, want_ne, f"NE {shape} {what}"), same(vb, want_vb, f"vb {shape} {what}")
        assert same_double(sse, want_sse) or (np.isnan(sse) and np.isnan(want_sse)), (shape, what, sse, want_sse)  # both add in pixel order
        same(capi.history_blend_adaptive_host(S, counts, cur), ref.blend(S, counts, cur), f"blend {shape} {what}")
        K, VK = capi.history_capture_adaptive_host(S, feat, noise, counts, cur, var)
        want_K, want_VK = ref.capture(S, feat, noise, counts, cur, var)
        same(K, want_K, f"K {shape} {what}"), same(VK, want_VK, f"VK {shape} {what}")
        same(K[0, :, 3], ne, "K0.w is NE"), same(VK, vb, "VK is pass A's vb")


def test_the_inputs_hold_the_cases_the_steps_branch_on():
    W, R = ref.SHAPES[0]
    counts, noise, S, feat, C, VC = inputs(W, R)
    th = C[:, 3]
    assert (th == 0).any() and (th == ref.CAP).any() and ((th > 0) & (th < ref.CAP)).any()
    idx = np.flatnonzero(th == 0)
    assert any(th[min(i + 1, th.size - 1)] == ref.CAP or th[max(i - 1, 0)] == ref.CAP for i in idx)  # a rejected lookup beside a capped one
    assert np.isnan(VC).any() and np.isinf(VC).any()
    w, ne, vb, sse = ref.noise_counts(noise, counts, C, VC)
    assert (noise[0, :, 3] == 0).any() and (noise[0, :, 3] > 0).any()  # zero-variance pixels among the others
    assert np.isnan(w).any() and np.isinf(w).any() and (w == 0).any()
    k = ref.keys_blend(w, ne, W, R)
    assert (k == 0xFFFFFFFF).any() and (k == 0x7F800000).any() and (k < 0x7F800000).any()  # a NaN key sorts first, an infinite one next


@pytest.mark.parametrize("shape", ref.SHAPES, ids=SHAPE_IDS)
def test_selection_equals_the_restatement(shape):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    W, R = shape
    n = W * R
    counts, noise, S, feat, C, VC = inputs(W, R)
    saw_more_than_cap = False
    for cur, var, what in ((None, None, "absent"), (C, VC, "present")):
        for name, thr in ref.thresholds(noise, counts, W, R, cur, var).items():
            for cap in ref.caps(n):
                got, above, m = capi.history_select_threshold_blend_host(noise, counts, W, R, thr, cap, cur, var)
                want, want_above, want_m = ref.select_threshold_blend(noise, counts, W, R, thr, cap, cur, var)
                assert (above, m) == (want_above, want_m) and m == min(above, cap), (shape, what, name, cap, above, m, want_above, want_m)
                assert np.array_equal(got, want), (shape, what, name, cap, got[:8], want[:8])
                saw_more_than_cap |= above > cap
    assert saw_more_than_cap


@pytest.mark.parametrize("shape", ref.SHAPES, ids=SHAPE_IDS)
def test_a_key_equal_to_the_threshold_is_not_above(shape):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    W, R = shape
    noise, counts, C, VC, thr = ref.tie_planes(W, R)
    w, ne, _, _ = ref.noise_counts(noise, counts, C, VC)
    k = ref.keys_blend(w, ne, W, R)
    tied = k == bits(np.array([f32(thr) * f32(thr)], f32))[0]
    hot = (np.arange(W * R) % 29 == 7).any()
    assert tied.any() and (not hot or (k[~tied] > k[tied][0]).all())
    got, above, m = capi.history_select_threshold_blend_host(noise, counts, W, R, thr, W * R, C, VC)
    want, want_above, want_m = ref.select_threshold_blend(noise, counts, W, R, thr, W * R, C, VC)
    assert (above, m) == (want_above, want_m) == (int((~tied).sum()), int((~tied).sum()))
    assert np.array_equal(got, want) and np.array_equal(got, np.flatnonzero(~tied))


@pytest.mark.parametrize("shape", ref.SHAPES, ids=SHAPE_IDS)
def test_filter_equals_the_restatement(shape):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    W, R = shape
    counts, noise, S, feat, C, VC = inputs(W, R)
    finite = tame(VC)
    for cur, var, what in ((None, None, "absent"), (C, finite, "present")):
        for opts in (dict(levels=2), dict(levels=1, keep_albedo=True, sigma_color=3.0)):
            stats = {}
            want = ref.denoise(S, feat, noise, counts, W, R, cur, var, stats=stats, **opts)
            same(capi.history_denoise_adaptive_host(S, feat, noise, counts, W, R, cur, var, **opts), want, f"filter {shape} {what} {opts}")
            raw, pre = capi.history_denoise_adaptive_variance_host(S, feat, noise, counts, W, R, cur, var, **opts)
            same(raw, stats["var_raw"], f"var_raw {shape} {what}"), same(pre, stats["var_0"], f"var_0 {shape} {what}")


@pytest.mark.parametrize("shape", ref.SHAPES, ids=SHAPE_IDS)
def test_without_history_the_steps_are_the_adaptive_ones(shape):
    """Identity (a), C absent: the keys are ptad::keys_host's, list, above and m pt_adaptive_select_threshold_host's, the resolve is
    S / Tf_p, the filter pt_denoise_adaptive_host's and W noise plane 0's .w."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    W, R = shape
    n = W * R
    counts, noise, S, feat, _, _ = inputs(W, R)
    w, ne, vb, _ = capi.history_noise_adaptive_host(noise, counts)
    same(w, noise[0, :, 3], "W is plane 0's .w"), same(ne, counts[:, 0].astype(f32), "NE is Tf")
    assert np.array_equal(ref.keys_blend(w, ne, W, R), adaptive_ref.keys(noise[0, :, 3], W, R, counts))
    for name, thr in ref.thresholds(noise, counts, W, R, None, None).items():
        for cap in ref.caps(n):
            got = capi.history_select_threshold_blend_host(noise, counts, W, R, thr, cap)
            want = capi.adaptive_select_threshold_host(noise, counts, W, R, thr, cap)
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (shape, name, cap)
    with np.errstate(all="ignore"):
        same(capi.history_blend_adaptive_host(S, counts), (S / counts[:, 0:1].astype(f32)).astype(f32), "resolve")
    same(capi.history_denoise_adaptive_host(S, feat, noise, counts, W, R, levels=2), capi.denoise_adaptive_host(S, feat, noise, counts, W, R, levels=2), "filter")


@pytest.mark.parametrize("shape", ref.SHAPES, ids=SHAPE_IDS)
def test_with_uniform_counts_the_steps_are_the_history_ones(shape):
    """Identity (b), counts (T, M) everywhere and C, VC present: the blend is pt_history_blend_host((float)T)'s, K and VK
    pt_history_capture_host's and _capture_variance_host's, W pt_history_noise_host's."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    W, R = shape
    n = W * R
    T, M = 23, 5
    counts = ref.uniform_counts(n, T, M)
    noise, S = ref.noise_planes(counts)
    _, feat = denoise_ref.random_frame(W, R, 4)
    C, VC = ref.current_planes(n, 5 * n)
    same(capi.history_blend_adaptive_host(S, counts, C), capi.history_blend_host(S, float(T), C), "blend")
    K, VK = capi.history_capture_adaptive_host(S, feat, noise, counts, C, VC)
    same(K, capi.history_capture_host(S, feat, float(T), C), "K")
    same(VK, capi.history_capture_variance_host(noise, M, T, float(T), C, VC), "VK")
    w, ne, _, sse = capi.history_noise_adaptive_host(noise, counts, C, VC)
    want_w, want_sse = capi.history_noise_host(noise, M, T, float(T), C, VC)
    same(w, want_w, "W")
    assert same_double(sse, want_sse) or (np.isnan(sse) and np.isnan(want_sse))
    finite = tame(VC)
    raw, _ = capi.history_denoise_adaptive_variance_host(S, feat, noise, counts, W, R, C, finite, levels=1)
    import history_variance_ref as vref
    stats = {}
    vref.denoise_history(S, feat, noise, W, R, M, T, float(T), C, finite, levels=1, stats=stats)
    same(raw, stats["var_raw"], "var_raw is the history form's")


def test_host_refusals():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    W, R = 5, 3
    n = W * R
    counts = ref.random_counts(n)
    noise, S = ref.noise_planes(counts)
    _, feat = denoise_ref.random_frame(W, R, 4)
    C, VC = ref.current_planes(n, 1)

    def refused(call, *phrases):
        with pytest.raises(capi.PtError) as e:
            call()
        for p in phrases:
            assert p in str(e.value), (p, str(e.value))

    one_group, few_iters = counts.copy(), counts.copy()
    one_group[7] = (9, 1)
    few_iters[4] = (3, 4)
    calls = {
        "pt_history_noise_adaptive_host": lambda c, cur=None, var=None: capi.history_noise_adaptive_host(noise, c, cur, var),
        "pt_history_select_threshold_blend_host": lambda c, cur=None, var=None: capi.history_select_threshold_blend_host(noise, c, W, R, 0.1, 4, cur, var),
        "pt_history_capture_adaptive_host": lambda c, cur=None, var=None: capi.history_capture_adaptive_host(S, feat, noise, c, cur, var),
        "pt_history_denoise_adaptive_host": lambda c, cur=None, var=None: capi.history_denoise_adaptive_host(S, feat, noise, c, W, R, cur, var),
        "pt_history_denoise_adaptive_variance_host": lambda c, cur=None, var=None: capi.history_denoise_adaptive_variance_host(S, feat, noise, c, W, R, cur, var),
    }
    for who, call in calls.items():
        refused(lambda: call(one_group), who + ":", "pixel 7", "9", "1")
        refused(lambda: call(few_iters), who + ":", "pixel 4", "3", "4")
        refused(lambda: call(counts, C, None), who + ":", "variance")
        refused(lambda: call(counts, None, VC), who + ":", "variance")
        call(counts, C, VC)
    refused(lambda: capi.history_blend_adaptive_host(S, one_group), "pt_history_blend_adaptive_host:", "pixel 7")
    refused(lambda: capi.history_select_threshold_blend_host(noise, counts, W, R, -1.0, 4), "pt_history_select_threshold_blend_host:", "threshold")
    refused(lambda: capi.history_select_threshold_blend_host(noise, counts, W, R, float("nan"), 4), "pt_history_select_threshold_blend_host:", "threshold")
    refused(lambda: capi.history_denoise_adaptive_host(S, feat, noise, counts, W, R, levels=9), "pt_history_denoise_adaptive_host:", "levels")


def test_host_code_under_the_sanitizers(tmp_path):
    """pt_history.h and pt_denoise.h are plain C++: a stand-alone driver (tests/integration/history_threshold_driver.cpp) runs the host
    loops on the shapes above with address and undefined-behaviour checks, built by the system compiler and run directly."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no system C++ compiler on this machine")
    exe = str(tmp_path / "history_threshold_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
           "-I", CSRC, os.path.join(ROOT, "tests", "integration", "history_threshold_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr and "threshold: 24 cases" in r.stdout, (r.returncode, r.stdout, r.stderr)
