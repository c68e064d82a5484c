"""The feedback on the host (pt_history_reproject_feedback_host / pt_history_denoise_feedback_host: csrc/pt_history.h and
csrc/pt_denoise.h, the bodies the HIP kernels run too) against the numpy restatement tests/history_feedback_ref.py, bit for bit, and the
identities that tie the feedback to the moments form.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref
import history_feedback_ref as ref
import history_round_ref as rref
from history_ref import bits, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "csrc")
SPP = 1


def same(got, want, what=""):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


@pytest.mark.parametrize("motion", [False, True], ids=["still", "motion"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.SHAPE_IDS)
def test_lookup_with_feedback(shape, motion):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, rows, row0, frame_rows = shape
    cam, kept, feat, reject, table, kind, vk, fk = ref.lookup_arrays(*shape)
    mo = dict(table=table, kind=kind) if motion else {}
    for opts in (dict(), dict(cap=8.0, min_normal_dot=0.5, plane_tol=0.25)):
        C, VC, FC = capi.history_reproject_feedback_host(cam.to_capi(), kept, feat, reject, vk, fk, w, rows, row0, **mo, **opts)
        want = ref.reproject_feedback(cam, kept, feat, reject, vk, fk, w, rows, row0, **mo, **opts)
        for got, exp, what in zip((C, VC, FC), want, ("C", "VC", "FC")):
            same(got, exp, f"{what} {w}x{rows}")
        # the raw chain: C and VC are the moments lookup's, the same bits
        if motion:
            raw = capi.history_reproject_motion_host(cam.to_capi(), kept, feat, reject, table, kind, w, rows, row0, flags=capi.HISTORY_MOTION | capi.HISTORY_MOMENTS,
                                                     kept_var=vk, **opts)
        else:
            raw = capi.history_reproject_moments_host(cam.to_capi(), kept, feat, reject, vk, w, rows, row0, **opts)
        same(C, raw[0], "C is the moments lookup's"), same(VC, raw[1], "VC is the moments lookup's")
        assert not FC[C[:, 3] == 0].any()  # a rejected pixel carries nothing
        if w * rows > 100:
            carried = C[:, 3] > 0
            assert carried.any() and (FC[carried, :3] > 0).any() and (FC[carried, 3] > 0).any()
            if opts:  # the cap is reached and touches nothing of FC
                capped = C[:, 3] == f32(8.0)
                assert capped.any() and (FC[capped, 3] > 0).any()


def cases():
    for levels in (1, 2, 3):
        for level in sorted({1, levels}):
            for variance in (0, 1):
                yield levels, level, variance


@pytest.mark.parametrize("extras", [False, True], ids=["uniform", "counted"])
@pytest.mark.parametrize("levels,level,variance", list(cases()))
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.SHAPE_IDS)
def test_filter_with_feedback(shape, levels, level, variance, extras):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, rows = shape[:2]
    n = w * rows
    S, planes = denoise_ref.random_frame(w, rows, SPP)
    C, VC, FC = ref.current_planes(n, 3 * n + levels)
    E = ref.extra_plane(n, n) if extras else None
    for keep in (False, True):
        opts = dict(levels=levels, keep_albedo=keep)
        st, got_st = {}, {}
        want, want_P = ref.denoise_feedback(S, planes, w, rows, SPP, E, C, VC, FC, level, variance, stats=st, **opts)
        got, P = capi.history_denoise_feedback_host(S, planes, w, rows, SPP, E, C, VC, FC, level=level, variance=variance, stats=got_st, **opts)
        same(got, want, "the filtered image"), same(P, want_P, "the tap")
        assert np.array_equal(got_st["mark"], st["mark"])
        same(got_st["var_raw"], st["var_raw"], "var_raw after the spatial step")
        assert not (got_st["var_raw"] < 0).any()  # no mark is left behind
        # the tap's xyz are the output of the same filter run with levels = L
        short, short_P = capi.history_denoise_feedback_host(S, planes, w, rows, SPP, E, C, VC, FC, level=level, variance=variance, levels=level, keep_albedo=keep)
        same(P[:, :3], short, "the tap's xyz: the filter with levels = L"), same(P, short_P, "the tap does not depend on the levels behind it")
        if level == levels:
            same(P[:, :3], got, "L == levels: the tap's xyz equal the output")
        # variance == 0: var_raw and the marks are the moments form's, from the raw chain
        if variance == 0:
            mst = {}
            if extras:
                capi.history_denoise_moments_counted_host(S, planes, w, rows, SPP, E, C, VC, stats=mst, **opts)
            else:
                capi.history_denoise_moments_host(S, planes, w, rows, SPP, C, VC, stats=mst, **opts)
            assert np.array_equal(got_st["mark"], mst["mark"])
            unmarked = ~mst["mark"]  # (a marked pixel's estimate reads the colour that is filtered, which differs)
            same(got_st["var_raw"][unmarked], mst["var_raw"][unmarked], "var_raw is the moments form's")
        if n > 100:
            assert st["mark"].any() and not st["mark"].all() and (st["var_raw"][~st["mark"]] > 0).any()
            assert (P[:, 3] > 0).any() and np.isfinite(P).all()


@pytest.mark.parametrize("variance", [0, 1])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.SHAPE_IDS)
def test_without_history_it_is_the_moments_filter(shape, variance):
    """FC absent (and C with it): the colour is S / ns and every pixel is marked under either rule, so the output is the moments form's."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, rows = shape[:2]
    S, planes = denoise_ref.random_frame(w, rows, SPP)
    E = ref.extra_plane(w * rows, 5)
    for levels in (1, 2, 3):
        got, P = capi.history_denoise_feedback_host(S, planes, w, rows, SPP, level=levels, variance=variance, levels=levels)
        same(got, capi.history_denoise_moments_host(S, planes, w, rows, SPP, levels=levels), "uniform")
        same(P[:, :3], got)
        got, _ = capi.history_denoise_feedback_host(S, planes, w, rows, SPP, E, level=1, variance=variance, levels=levels)
        same(got, capi.history_denoise_moments_counted_host(S, planes, w, rows, SPP, E, levels=levels), "counted")
        same(got, rref.denoise_moments(S, planes, w, rows, SPP, E, levels=levels), "... and the restatement's")


def test_feedback_of_the_raw_blend_changes_nothing():
    """FC.xyz = C.xyz: the colour that is filtered is the raw blend, so rule 0 gives the moments form's output, bit for bit."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, rows = ref.SHAPES[0][:2]
    S, planes = denoise_ref.random_frame(w, rows, SPP)
    C, VC, FC = ref.current_planes(w * rows, 11)
    FC[:, :3] = C[:, :3]
    got, _ = capi.history_denoise_feedback_host(S, planes, w, rows, SPP, None, C, VC, FC, levels=2, variance=0)
    same(got, capi.history_denoise_moments_host(S, planes, w, rows, SPP, C, VC, levels=2))
    other, _ = capi.history_denoise_feedback_host(S, planes, w, rows, SPP, None, C, VC, FC, levels=2, variance=1)
    assert not np.array_equal(bits(other), bits(got))  # rule 1 reads FC.w


def test_host_refusals():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, rows, row0, frame_rows = ref.SHAPES[2]
    n = w * rows
    cam, kept, feat, reject, table, kind, vk, fk = ref.lookup_arrays(*ref.SHAPES[2])
    S, planes = denoise_ref.random_frame(w, rows, SPP)
    C, VC, FC = ref.current_planes(n, 1)

    def refused(call, *phrases):
        with pytest.raises(capi.PtError) as e:
            call()
        for p in phrases:
            assert p in str(e.value), (p, str(e.value))

    who = "pt_history_reproject_feedback_host"
    cc = cam.to_capi()
    refused(lambda: capi.history_reproject_feedback_host(cc, kept, feat, reject, vk, fk, w, rows, frame_rows), who, "kept camera")
    refused(lambda: capi.history_reproject_feedback_host(cc, kept, feat, reject, vk, fk, w, rows, 0, cap=-1.0), who, "cap")
    refused(lambda: capi.history_reproject_feedback_host(cc, kept, feat, reject, vk, fk, w, rows, 0, table=table, kind=np.full(kind.size, 3, np.uint8)), who, "kind[0]")
    L = capi.lib()
    out = np.empty((n, 4), np.float32)
    assert L.pt_history_reproject_feedback_host(w, rows, 0, cc, capi._f(kept), capi._f(feat), None, 0, None, capi._f(vk), None, None, None, capi._f(out), capi._f(out),
                                                capi._f(out)) != 0
    assert who in L.pt_last_error().decode() and "null" in L.pt_last_error().decode()

    who = "pt_history_denoise_feedback_host"
    # the moments form's refusals first, in their order: samples, the options, C without VC; then fb, then C without FC
    refused(lambda: capi.history_denoise_feedback_host(S, planes, w, rows, 0.0, None, C, None, None, level=9, levels=9), who, "samples")
    refused(lambda: capi.history_denoise_feedback_host(S, planes, w, rows, 1.0, None, C, None, None, level=9, levels=9), who, "levels")
    refused(lambda: capi.history_denoise_feedback_host(S, planes, w, rows, 1.0, None, C, None, None, level=9), who, "moments")
    refused(lambda: capi.history_denoise_feedback_host(S, planes, w, rows, 1.0, None, C, VC, None, level=6), who, "feedback level 6", "1 .. 5")
    refused(lambda: capi.history_denoise_feedback_host(S, planes, w, rows, 1.0, None, C, VC, None, level=3, levels=2), who, "feedback level 3", "1 .. 2")
    refused(lambda: capi.history_denoise_feedback_host(S, planes, w, rows, 1.0, None, C, VC, None, level=-1), who, "feedback level")
    refused(lambda: capi.history_denoise_feedback_host(S, planes, w, rows, 1.0, None, C, VC, None, variance=2), who, "feedback variance 2")
    refused(lambda: capi.history_denoise_feedback_host(S, planes, w, rows, 1.0, None, C, VC, None, variance=-2), who, "feedback variance -2")
    refused(lambda: capi.history_denoise_feedback_host(S, planes, w, rows, 1.0, None, C, VC, None), who, "filtered colour")
    refused(lambda: capi.history_denoise_feedback_host(S, planes, w, rows, 1.0, None, None, None, FC), who, "filtered colour")
    refused(lambda: capi.history_denoise_feedback_host(S, planes, w, rows, 1.0, np.full(n, -1.0, np.float32), C, VC, FC), who, "extra")
    # the defaults: level 1 and rule 1; the field's -1 is rule 0
    got = capi.history_denoise_feedback_host(S, planes, w, rows, 1.0, None, C, VC, FC)
    for a, b in zip(got, capi.history_denoise_feedback_host(S, planes, w, rows, 1.0, None, C, VC, FC, level=1, variance=1)):
        same(a, b, "the defaults")
    assert capi.history_feedback_options(0, 0).variance == -1 and capi.history_feedback_options().variance == 0


def test_host_code_under_the_sanitizers(tmp_path):
    """pt_history.h and pt_denoise.h are plain C++: a stand-alone driver (tests/integration/history_feedback_driver.cpp) runs the loops
    above once — shapes, levels, tap levels, rules, extras, motion — with address and undefined-behaviour checks, built by the system
    compiler and run directly."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no system C++ compiler on this machine")
    exe = str(tmp_path / "history_feedback_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
           "-I", CSRC, os.path.join(ROOT, "tests", "integration", "history_feedback_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr and "feedback: 144 cases" in r.stdout, (r.returncode, r.stdout, r.stderr)
