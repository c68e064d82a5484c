"""The variance side of the reprojected history and the filter over the blend on the host (pt_history_capture_variance_host /
_reproject_variance_host / _denoise_host: csrc/pt_history.h and csrc/pt_denoise.h, the bodies the HIP kernels run too) against the
numpy restatement tests/history_variance_ref.py, bit for bit.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_guided_ref
import denoise_ref
import history_ref as href
import history_variance_ref as ref
from history_ref import bits, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "csrc")
GROUPS, ITERS = 3, 4  # of the made-up folds: T = 4 iterations in M = 3 groups


def same(got, want, what=""):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


def kept_variance(n, seed):
    """VK [n, 4]: variances many decades apart, zeros among them, .w = +0."""
    rng = np.random.default_rng(seed)
    vk = np.zeros((n, 4), f32)
    vk[:, :3] = (rng.random((n, 3), dtype=f32) * f32(10.0) ** rng.integers(-12, 1, (n, 3)).astype(f32)).astype(f32)
    vk[rng.random(n) < 0.15, :3] = 0
    return vk


def current_planes(n, seed, cap=32.0):
    """C, VC [n, 4] of a lookup that carried most pixels: weights up to the cap (reached by a fifth), rejected pixels all zero."""
    rng = np.random.default_rng(seed)
    C, VC = np.zeros((n, 4), f32), kept_variance(n, seed + 1)
    C[:, :3] = rng.random((n, 3), dtype=f32)
    C[:, 3] = (rng.random(n, dtype=f32) * f32(cap)).astype(f32)
    C[rng.random(n) < 0.2, 3] = cap
    gone = rng.random(n) < 0.25
    C[gone], VC[gone] = 0, 0
    return C, VC


@pytest.mark.parametrize("name", sorted(href.OPTION_SETS))
@pytest.mark.parametrize("row0", [7])
@pytest.mark.parametrize("w,rows", href.SHAPES)
def test_lookup_with_variance_on_adversarial_arrays(w, rows, row0, name):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    cam, kept, feat, reject, _ = href.adversarial(w, rows, row0)
    opts = href.OPTION_SETS[name]
    vk = kept_variance(w * rows, 10 * w + rows)
    C, VC = capi.history_reproject_variance_host(cam.to_capi(), kept, feat, reject, vk, w, rows, row0, **opts)
    want_C, want_VC = ref.reproject_variance(cam, kept, feat, reject, vk, w, rows, row0, **opts)
    assert np.isfinite(want_VC).all()
    same(C, want_C, f"C {w}x{rows} {name}")
    same(VC, want_VC, f"VC {w}x{rows} {name}")
    same(C, capi.history_reproject_host(cam.to_capi(), kept, feat, reject, w, rows, row0, **opts), "C is the plain lookup's")
    assert not VC[C[:, 3] == 0].any() and not VC[:, 3].any()  # a rejected pixel carries no variance; .w stays +0
    if w * rows > 100:
        assert (VC[:, :3] > 0).any() and ((C[:, 3] > 0) & ~VC[:, :3].any(axis=1)).any()  # carried with and without variance
        if name == "custom":  # the cap is reached and does not touch vh
            capped = C[:, 3] == f32(8.0)
            assert capped.any() and (VC[capped, :3] > 0).any()


@pytest.mark.parametrize("w,rows", href.SHAPES)
def test_capture_with_variance(w, rows):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = w * rows
    noise = denoise_guided_ref.random_noise_planes(w, rows, GROUPS, ITERS)
    vn = ref.sample_variance(noise, GROUPS, ITERS)
    same(capi.history_capture_variance_host(noise, GROUPS, ITERS, ITERS), ref.capture_variance(noise, GROUPS, ITERS, ITERS), "C absent")
    same(capi.history_capture_variance_host(noise, GROUPS, ITERS, ITERS)[:, :3], vn, "C absent: the variance of the new samples")
    C, VC = current_planes(n, n)
    got = capi.history_capture_variance_host(noise, GROUPS, ITERS, ITERS, C, VC)
    same(got, ref.capture_variance(noise, GROUPS, ITERS, ITERS, C, VC), "C present")
    gone = C[:, 3] == 0
    same(got[gone, :3], vn[gone], "a rejected pixel starts again from the view's own estimate")
    assert not got[:, 3].any()
    if n > 100:
        assert (vn == 0).all(axis=1).any() and (C[:, 3] == f32(32.0)).any()  # a zero-variance pixel, the cap reached
        both_zero = (vn == 0).all(axis=1) & ~VC[:, :3].any(axis=1)
        assert both_zero.any() and not got[both_zero].any()


@pytest.mark.parametrize("opts", [dict(), dict(keep_albedo=True), dict(levels=2, sigma_color=2.0, sigma_normal=-1.0)], ids=["defaults", "keep_albedo", "custom"])
@pytest.mark.parametrize("w,rows", href.SHAPES)
def test_filter_over_the_blend(w, rows, opts):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = w * rows
    _, planes = denoise_ref.random_frame(w, rows, ITERS)
    noise = denoise_guided_ref.random_noise_planes(w, rows, GROUPS, ITERS)
    S = noise[0, :, :3]  # the fold keeps prev == S
    C, VC = current_planes(n, 3 * n)
    st = {}
    want = ref.denoise_history(S, planes, noise, w, rows, GROUPS, ITERS, ITERS, C, VC, stats=st, **opts)
    same(capi.history_denoise_host(S, planes, noise, w, rows, GROUPS, ITERS, ITERS, C, VC, **opts), want, f"{w}x{rows}")
    same(capi.history_denoise_host(S, planes, noise, w, rows, GROUPS, ITERS, ITERS, **opts),
         ref.denoise_history(S, planes, noise, w, rows, GROUPS, ITERS, ITERS, **opts), f"{w}x{rows}, C absent")
    if n > 100:
        assert (st["var_raw"] == 0).any() and (st["var_raw"] > 0).any()


@pytest.mark.parametrize("opts", [dict(), dict(keep_albedo=True)], ids=["defaults", "keep_albedo"])
@pytest.mark.parametrize("w,rows", href.SHAPES)
def test_without_history_it_is_the_guided_filter(w, rows, opts):
    """C and VC absent, samples == (float)T, S >= 0: wn = 1, wh = 0, vb = vn, and the blend is S / T."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    _, planes = denoise_ref.random_frame(w, rows, ITERS)
    noise = denoise_guided_ref.random_noise_planes(w, rows, GROUPS, ITERS)
    S = noise[0, :, :3]
    assert (S >= 0).all()
    same(capi.history_denoise_host(S, planes, noise, w, rows, GROUPS, ITERS, ITERS, **opts),
         capi.denoise_guided_host(S, planes, noise, w, rows, GROUPS, ITERS, **opts), f"{w}x{rows}")


def test_host_refusals():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, rows = 5, 3
    n = w * rows
    cam, kept, feat, reject, _ = href.adversarial(w, rows, 0)
    _, planes = denoise_ref.random_frame(w, rows, ITERS)
    noise = denoise_guided_ref.random_noise_planes(w, rows, GROUPS, ITERS)
    S = noise[0, :, :3]
    C, VC = current_planes(n, 1)
    vk = kept_variance(n, 2)

    def refused(call, *phrases):
        with pytest.raises(capi.PtError) as e:
            call()
        for p in phrases:
            assert p in str(e.value), (p, str(e.value))

    who = "pt_history_capture_variance_host"
    for samples in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: capi.history_capture_variance_host(noise, GROUPS, ITERS, samples), who, "samples")
    refused(lambda: capi.history_capture_variance_host(noise, 1, ITERS, ITERS), who, "at least 2")
    refused(lambda: capi.history_capture_variance_host(noise, 5, ITERS, ITERS), who, "5 groups cannot hold 4")
    refused(lambda: capi.history_capture_variance_host(noise, GROUPS, ITERS, 3.0), who, "samples 3", "4 iterations")
    refused(lambda: capi.history_capture_variance_host(noise, GROUPS, ITERS, ITERS, C, None), who, "variance")
    refused(lambda: capi.history_capture_variance_host(noise, GROUPS, ITERS, ITERS, None, VC), who, "variance")

    who = "pt_history_reproject_variance_host"
    refused(lambda: capi.history_reproject_variance_host(cam.to_capi(), kept, feat, reject, vk, w, rows, 4), who, "kept camera")
    refused(lambda: capi.history_reproject_variance_host(cam.to_capi(), kept, feat, reject, vk, w, rows, 0, cap=-1.0), who, "cap")
    refused(lambda: capi.history_reproject_variance_host(cam.to_capi(), kept, feat, reject, vk, w, rows, 0, plane_tol=float("inf")), who, "finite")

    who = "pt_history_denoise_host"
    ok = (S, planes, noise, w, rows, GROUPS, ITERS, ITERS)
    # in pt_history_denoise's order: samples, the options, the folds' counters, samples against them, C without VC
    refused(lambda: capi.history_denoise_host(S, planes, noise, w, rows, 1, ITERS, 0.0, C, None, levels=9), who, "samples")
    refused(lambda: capi.history_denoise_host(S, planes, noise, w, rows, 1, ITERS, 3.0, C, None, levels=9), who, "levels")
    refused(lambda: capi.history_denoise_host(*ok, sigma_color=float("nan")), who, "sigma")
    refused(lambda: capi.history_denoise_host(S, planes, noise, w, rows, 1, ITERS, 3.0, C, None), who, "at least 2")
    refused(lambda: capi.history_denoise_host(S, planes, noise, w, rows, 5, ITERS, 3.0, C, None), who, "cannot hold")
    refused(lambda: capi.history_denoise_host(S, planes, noise, w, rows, GROUPS, ITERS, 3.0, C, None), who, "samples 3")
    refused(lambda: capi.history_denoise_host(*ok, C, None), who, "variance")
    refused(lambda: capi.history_denoise_host(*ok, None, VC), who, "variance")
    capi.history_denoise_host(*ok, C, VC)


@pytest.mark.parametrize("w,rows", [(5, 3), (97, 61)])
def test_host_code_under_the_sanitizers(tmp_path, w, rows):
    """pt_history.h and pt_denoise.h are plain C++: a stand-alone driver (tests/integration/history_variance_driver.cpp) runs capture,
    lookup and filter with address and undefined-behaviour checks, built by the system compiler and run directly."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no system C++ compiler on this machine")
    exe = str(tmp_path / "history_variance_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
           "-I", CSRC, os.path.join(ROOT, "tests", "integration", "history_variance_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(w), str(rows)], capture_output=True, text=True)
    assert r.returncode == 0 and "carried" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)
    carried = int(r.stdout.split(":")[1].split()[0])
    assert 0 < carried < w * rows
