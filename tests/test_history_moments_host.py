"""Moments with the history on the host (pt_history_capture_moments_host / _reproject_moments_host / _denoise_moments_host:
csrc/pt_history.h and csrc/pt_denoise.h, the bodies the HIP kernels run too) against the numpy restatement
tests/history_moments_ref.py, bit for bit.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref
import history_ref as href
import history_moments_ref as ref
from history_ref import bits, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "csrc")
SPP = 1  # the case the moments exist for


def same(got, want, what=""):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


def kept_moments(n, seed):
    """VK [n, 4]: second moments many decades apart, zeros among them; r between 1/32 and 1."""
    rng = np.random.default_rng(seed)
    vk = np.zeros((n, 4), f32)
    vk[:, :3] = (rng.random((n, 3), dtype=f32) * f32(10.0) ** rng.integers(-12, 1, (n, 3)).astype(f32)).astype(f32)
    vk[rng.random(n) < 0.15, :3] = 0
    vk[:, 3] = rng.choice(np.array([1.0, 0.5, 0.3, 0.25, 0.125, 0.03125], f32), n)
    return vk


def current_planes(n, seed, cap=32.0):
    """C, VC [n, 4] of a lookup that carried most pixels: weights up to the cap (reached by a fifth), rejected pixels all zero."""
    rng = np.random.default_rng(seed)
    C, VC = np.zeros((n, 4), f32), kept_moments(n, seed + 1)
    C[:, :3] = rng.random((n, 3), dtype=f32)
    C[:, 3] = (rng.random(n, dtype=f32) * f32(cap)).astype(f32)
    C[rng.random(n) < 0.2, 3] = cap
    gone = rng.random(n) < 0.25
    C[gone], VC[gone] = 0, 0
    return C, VC


@pytest.mark.parametrize("name", sorted(href.OPTION_SETS))
@pytest.mark.parametrize("row0", [7])
@pytest.mark.parametrize("w,rows", href.SHAPES)
def test_lookup_with_moments_on_adversarial_arrays(w, rows, row0, name):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    cam, kept, feat, reject, _ = href.adversarial(w, rows, row0)
    opts = href.OPTION_SETS[name]
    vk = kept_moments(w * rows, 10 * w + rows)
    C, VC = capi.history_reproject_moments_host(cam.to_capi(), kept, feat, reject, vk, w, rows, row0, **opts)
    want_C, want_VC = ref.reproject_moments(cam, kept, feat, reject, vk, w, rows, row0, **opts)
    assert np.isfinite(want_VC).all()
    same(C, want_C, f"C {w}x{rows} {name}")
    same(VC, want_VC, f"VC {w}x{rows} {name}")
    same(C, capi.history_reproject_host(cam.to_capi(), kept, feat, reject, w, rows, row0, **opts), "C is the plain lookup's")
    assert not VC[C[:, 3] == 0].any()  # a rejected pixel carries nothing
    if w * rows > 100:
        carried = C[:, 3] > 0
        assert (VC[carried, 3] > 0).all() and (VC[carried, 3] <= 1).all()  # r is interpolated with the rest: a convex mix of the taps'
        assert (VC[:, :3] > 0).any() and len(np.unique(VC[carried, 3])) > 6
        if name == "custom":  # the cap is reached and touches neither m2h nor rh
            capped = C[:, 3] == f32(8.0)
            assert capped.any() and (VC[capped, :3] > 0).any() and (VC[capped, 3] > 0).all()


@pytest.mark.parametrize("w,rows", href.SHAPES)
def test_capture_with_moments(w, rows):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = w * rows
    S, planes = denoise_ref.random_frame(w, rows, SPP)
    for spp in (1, 4):
        got = capi.history_capture_moments_host(S, spp)
        same(got, ref.capture_moments(S, spp), "C absent")
        x = (np.asarray(S, f32).reshape(-1, 3) / f32(spp)).astype(f32)
        same(got[:, :3], x * x, "C absent: the square of the view's mean")
        assert (got[:, 3] == 1).all()  # one view: r = 1
        C, VC = current_planes(n, n + spp)
        got = capi.history_capture_moments_host(S, spp, C, VC)
        same(got, ref.capture_moments(S, spp, C, VC), "C present")
        gone = C[:, 3] == 0
        same(got[gone, :3], (x * x)[gone], "a rejected pixel starts again")
        assert (got[gone, 3] == 1).all()
    same(capi.history_capture_host(S, planes, SPP, C), href.capture(S, planes, SPP, C), "K is the plain capture's: the moments side has no part in it")
    # L equal views blended one after the other leave r = 1/L (to rounding: every step is a handful of float32 operations)
    r = np.ones((n, 4), f32)
    Cn = np.zeros((n, 4), f32)
    for L in range(2, 9):
        Cn[:, 3] = L - 1
        r = capi.history_capture_moments_host(S, 1, Cn, r)
        assert np.allclose(r[:, 3], 1.0 / L, rtol=1e-6, atol=0), L
    assert (r[:, 3] <= ref.R_MAX).all()  # ... and from the fourth on it is below the threshold


OPTION_SETS = [dict(), dict(keep_albedo=True), dict(levels=2, sigma_color=2.0, sigma_normal=-1.0), dict(levels=1, sigma_position=-1.0),
               dict(levels=1, sigma_normal=-1.0, sigma_position=-1.0)]
OPTION_IDS = ["defaults", "keep_albedo", "custom_no_normal", "no_position", "neither"]


@pytest.mark.parametrize("opts", OPTION_SETS, ids=OPTION_IDS)
@pytest.mark.parametrize("w,rows", href.SHAPES)
def test_filter_with_moments(w, rows, opts):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = w * rows
    S, planes = denoise_ref.random_frame(w, rows, SPP)
    C, VC = current_planes(n, 3 * n)
    st, got_st = {}, {}
    want = ref.denoise_moments(S, planes, w, rows, SPP, C, VC, stats=st, **opts)
    same(capi.history_denoise_moments_host(S, planes, w, rows, SPP, C, VC, stats=got_st, **opts), want, f"{w}x{rows}")
    assert np.array_equal(got_st["mark"], st["mark"])
    same(got_st["var_raw"], st["var_raw"], "var_raw after the spatial step")
    assert not (got_st["var_raw"] < 0).any()  # no mark is left behind
    if n > 100:
        assert st["mark"].any() and not st["mark"].all() and (st["var_raw"][~st["mark"]] > 0).any()
        assert (st["var_raw"][st["mark"]] > 0).any()


@pytest.mark.parametrize("pattern", ref.MARK_PATTERNS)
@pytest.mark.parametrize("w,rows", href.SHAPES)
def test_filter_on_the_mark_patterns(w, rows, pattern):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    S, planes = denoise_ref.random_frame(w, rows, SPP)
    C, VC, marked = ref.current_planes(w, rows, pattern)
    st, got_st = {}, {}
    want = ref.denoise_moments(S, planes, w, rows, SPP, C, VC, levels=2, stats=st)
    same(capi.history_denoise_moments_host(S, planes, w, rows, SPP, C, VC, levels=2, stats=got_st), want, f"{w}x{rows} {pattern}")
    assert np.array_equal(st["mark"], marked) and np.array_equal(got_st["mark"], marked)
    same(got_st["var_raw"], st["var_raw"], "var_raw after the spatial step")


@pytest.mark.parametrize("opts", [dict(), dict(keep_albedo=True)], ids=["defaults", "keep_albedo"])
@pytest.mark.parametrize("w,rows", href.SHAPES)
def test_without_history_every_pixel_is_marked(w, rows, opts):
    """C absent: rb = 1 for every pixel, so every pixel — the hit ones among them — is marked, and the capture gives VK = {x^2, 1}."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    S, planes = denoise_ref.random_frame(w, rows, SPP)
    st, got_st = {}, {}
    want = ref.denoise_moments(S, planes, w, rows, SPP, stats=st, **opts)
    same(capi.history_denoise_moments_host(S, planes, w, rows, SPP, stats=got_st, **opts), want, f"{w}x{rows}, C absent")
    assert got_st["mark"].all() and got_st["mark"][st["hit"]].all()
    same(got_st["var_raw"], st["var_raw"], "the spatial estimate of every pixel")
    vk = capi.history_capture_moments_host(S, SPP)
    x = (np.asarray(S, f32).reshape(-1, 3) / f32(SPP)).astype(f32)
    same(vk[:, :3], x * x, "m2 of one view")
    assert (vk[:, 3] == 1).all()


def test_the_threshold_is_inclusive():
    """samples = Th = 1: wn = wh = 1/2 and rb = 1/4 + rh / 4, exact for rh = 4 (t - 1/4) with t the threshold or the float above it."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, rows = 5, 3
    n = w * rows
    S, planes = denoise_ref.random_frame(w, rows, SPP)
    t = capi.HISTORY_MOMENTS_R_MAX
    assert t == ref.R_MAX
    above = np.nextafter(t, f32(1))
    C, VC = np.zeros((n, 4), f32), np.zeros((n, 4), f32)
    C[:, :3], C[:, 3] = 0.5, 1.0
    VC[:, :3] = 0.5
    VC[:, 3] = (t - f32(0.25)) * f32(4)
    VC[1::2, 3] = (above - f32(0.25)) * f32(4)
    rb = capi.history_capture_moments_host(S, 1, C, VC)[:, 3]
    assert (rb[0::2] == t).all() and (rb[1::2] == above).all()
    st = {}
    got = capi.history_denoise_moments_host(S, planes, w, rows, 1, C, VC, stats=st)
    assert not st["mark"][0::2].any() and st["mark"][1::2].all()
    same(got, ref.denoise_moments(S, planes, w, rows, 1, C, VC), "either side of the threshold")


def test_host_refusals():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, rows = 5, 3
    n = w * rows
    cam, kept, feat, reject, _ = href.adversarial(w, rows, 0)
    S, planes = denoise_ref.random_frame(w, rows, SPP)
    C, VC = current_planes(n, 1)
    vk = kept_moments(n, 2)

    def refused(call, *phrases):
        with pytest.raises(capi.PtError) as e:
            call()
        for p in phrases:
            assert p in str(e.value), (p, str(e.value))

    who = "pt_history_capture_moments_host"
    for samples in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: capi.history_capture_moments_host(S, samples), who, "samples")
    refused(lambda: capi.history_capture_moments_host(S, 1, C, None), who, "moments")
    refused(lambda: capi.history_capture_moments_host(S, 1, None, VC), who, "moments")

    who = "pt_history_reproject_moments_host"
    refused(lambda: capi.history_reproject_moments_host(cam.to_capi(), kept, feat, reject, vk, w, rows, 4), who, "kept camera")
    refused(lambda: capi.history_reproject_moments_host(cam.to_capi(), kept, feat, reject, vk, w, rows, 0, cap=-1.0), who, "cap")
    refused(lambda: capi.history_reproject_moments_host(cam.to_capi(), kept, feat, reject, vk, w, rows, 0, plane_tol=float("inf")), who, "finite")

    who = "pt_history_denoise_moments_host"
    # in pt_history_denoise_ex's order: samples, the options, C without VC
    refused(lambda: capi.history_denoise_moments_host(S, planes, w, rows, 0.0, C, None, levels=9), who, "samples")
    refused(lambda: capi.history_denoise_moments_host(S, planes, w, rows, 1.0, C, None, levels=9), who, "levels")
    refused(lambda: capi.history_denoise_moments_host(S, planes, w, rows, 1.0, C, None, sigma_color=float("nan")), who, "sigma")
    refused(lambda: capi.history_denoise_moments_host(S, planes, w, rows, 1.0, C, None), who, "moments")
    refused(lambda: capi.history_denoise_moments_host(S, planes, w, rows, 1.0, None, VC), who, "moments")
    capi.history_denoise_moments_host(S, planes, w, rows, 1.0, C, VC)


@pytest.mark.parametrize("w,rows", [(5, 3), (97, 61)])
def test_host_code_under_the_sanitizers(tmp_path, w, rows):
    """pt_history.h and pt_denoise.h are plain C++: a stand-alone driver (tests/integration/history_moments_driver.cpp) runs capture,
    lookup and filter over five views with address and undefined-behaviour checks, built by the system compiler and run directly."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no system C++ compiler on this machine")
    exe = str(tmp_path / "history_moments_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
           "-I", CSRC, os.path.join(ROOT, "tests", "integration", "history_moments_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(w), str(rows)], capture_output=True, text=True)
    assert r.returncode == 0 and "marked" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)
    first, last = (int(t.split()[0]) for t in r.stdout.split("marked:")[1].split(",")[:2])
    assert first == w * rows and 0 < last <= first  # every pixel on the first view; the miss always
    if w * rows > 100:
        assert last < first // 2  # ... and few once the history is long enough
