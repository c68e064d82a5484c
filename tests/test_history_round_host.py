"""The history round on the host (no GPU): pt_history_select_host, pt_history_merge_host and the counted twins of the blend, the
capture, the moments and the moments filter against tests/history_round_ref.py, bit for bit; their refusals; and the host loops under
the sanitizers in a stand-alone program (tests/integration/history_round_driver.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref
import history_moments_ref as mref
import history_round_ref as ref
from history_round_ref import bits, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "csrc")


def same(got, want, what=""):
    assert np.array_equal(bits(got), bits(want)), what


def check_select(feat, C, w, rows, **kw):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    want, fresh, m = ref.select(feat, C, ref.EMITTER, **kw)
    lst, got_fresh, got_m = capi.history_select_host(feat, w, rows, C, ref.EMITTER, **kw)
    assert (got_fresh, got_m) == (fresh, m), (kw, got_fresh, got_m, fresh, m)
    assert lst.size == ref.list_capacity(kw.get("max_fraction", 0.0), w * rows)
    assert np.array_equal(lst[:m], want), kw
    assert (lst[m:] == -1).all()  # the entries behind m keep what they held
    return fresh, m


@pytest.mark.parametrize("w,rows", ref.SHAPES)
def test_select_equals_the_restatement(w, rows):
    """The weights present are 0, 1, 2.5, 4, 7, 32: min_history between them (3), equal to some (4, 2.5, 1), below all but 0 (0.5);
    C absent: every non-emitter hit pixel with a known id is fresh."""
    feat, C = ref.random_planes(w, rows)
    n = w * rows
    ids = np.ascontiguousarray(feat[2, :, 3]).view(np.int32)
    hit = feat[1, :, 3] > 0
    eligible = hit & (ids >= 1) & (ids <= ref.NUM_GEOMS)
    eligible[eligible] = ref.EMITTER[ids[eligible] - 1] == 0
    fresh, m = check_select(feat, None, w, rows)
    assert fresh == m == int(eligible.sum())
    for mh in (0.0, 3.0, 4.0, 2.5, 1.0, 0.5):
        fresh, m = check_select(feat, C, w, rows, min_history=mh)
        want = eligible & (C[:, 3] < (mh or 4.0))
        assert fresh == m == int(want.sum())
    if n > 100:
        assert 0 < fresh < int(eligible.sum())  # misses, emitters, ids 0 and NUM_GEOMS + 1 and long histories were all present
        assert (~hit).any() and (ids == 0).any() and (ids == ref.NUM_GEOMS + 1).any() and (ids[hit] == 2).any()


@pytest.mark.parametrize("w,rows", ref.SHAPES)
def test_select_under_a_cap(w, rows):
    """fresh > cap, fresh == cap and fresh == 0; two weights only, so that the cut falls into a run of equal keys: the smaller index wins."""
    feat, C = ref.random_planes(w, rows, seed=1, weights=(1.0, 2.0))
    n = w * rows
    fresh, _ = check_select(feat, C, w, rows)
    if fresh > 1:
        for cap in (1, fresh // 2, fresh - 1, fresh):
            got_fresh, m = check_select(feat, C, w, rows, max_fraction=max(cap, 1) / n)
            assert got_fresh == fresh and m == min(fresh, ref.list_capacity(max(cap, 1) / n, n))
        key = ref.keys(feat, C, ref.EMITTER)
        top = int((key == key.max()).sum())
        for cap in {max(top // 2, 1), top + (fresh - top) // 2}:  # inside the run of the largest key, and of the second
            if cap in (top, fresh):
                continue
            check_select(feat, C, w, rows, max_fraction=cap / n)
            lst, _, m = ref.select(feat, C, ref.EMITTER, max_fraction=cap / n)
            ties = np.flatnonzero(key == key[lst].min())
            taken = np.isin(ties, lst)
            assert not taken.all() and taken[:taken.sum()].all()  # the cut lies inside a run of equal keys, and takes its front
    C[:, 3] = 4.0
    assert check_select(feat, C, w, rows) == (0, 0)
    assert check_select(feat, C, w, rows, max_fraction=0.25) == (0, 0)


@pytest.mark.parametrize("w,rows", ref.SHAPES)
def test_merge_equals_the_restatement(w, rows):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = w * rows
    S, E = ref.random_image(n), ref.random_extra(n)
    rng = np.random.default_rng(n)
    for m in sorted({1, n}):
        lst = np.sort(rng.choice(n, m, replace=False)).astype(np.int32)
        Sw = ref.random_image(m, seed=3)
        want_S, want_E = ref.merge(S, E, lst, Sw, 4)
        got_S, got_E = capi.history_merge_host(S, E, lst, Sw, 4)
        same(got_S, want_S, f"S, m = {m}")
        same(got_E, want_E, f"E, m = {m}")
        rest = np.setdiff1d(np.arange(n), lst)
        same(got_S[rest], S[rest]), same(got_E[rest], E[rest])
        assert (got_E[lst] == E[lst] + 4).all()


def frame(w, rows, seed=0):
    n = w * rows
    S, planes = denoise_ref.random_frame(w, rows, 1)
    C, VC, _ = mref.current_planes(w, rows, "checkerboard", seed)
    return n, np.ascontiguousarray(S, f32), planes, C, VC


@pytest.mark.parametrize("w,rows", ref.SHAPES)
def test_counted_forms_with_no_extras_are_the_uncounted(w, rows):
    """samples + 0 == samples: with E all zero every counted host function gives its twin's result bit for bit."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n, S, planes, C, VC = frame(w, rows)
    E = np.zeros(n, f32)
    for samples in (1.0, 3.0):
        for c, vc in ((None, None), (C, VC)):
            same(capi.history_blend_counted_host(S, samples, E, c), capi.history_blend_host(S, samples, c), "blend")
            same(capi.history_capture_counted_host(S, planes, samples, E, c), capi.history_capture_host(S, planes, samples, c), "capture")
            same(capi.history_capture_moments_counted_host(S, samples, E, c, vc), capi.history_capture_moments_host(S, samples, c, vc), "moments")
            a, b = {}, {}
            same(capi.history_denoise_moments_counted_host(S, planes, w, rows, samples, E, c, vc, stats=a),
                 capi.history_denoise_moments_host(S, planes, w, rows, samples, c, vc, stats=b), "filter")
            same(a["var_raw"], b["var_raw"]), same(a["mark"], b["mark"])


@pytest.mark.parametrize("opts", [dict(), dict(keep_albedo=True, levels=2)], ids=["defaults", "keep_albedo"])
@pytest.mark.parametrize("w,rows", ref.SHAPES)
def test_counted_forms_equal_the_restatement(w, rows, opts):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n, S, planes, C, VC = frame(w, rows, seed=2)
    E = ref.random_extra(n, seed=w)
    for c, vc in ((None, None), (C, VC)):
        same(capi.history_blend_counted_host(S, 1.0, E, c), ref.blend(S, 1.0, E, c), "blend")
        same(capi.history_capture_counted_host(S, planes, 1.0, E, c), ref.capture(S, planes, 1.0, E, c), "capture")
        same(capi.history_capture_moments_counted_host(S, 1.0, E, c, vc), ref.capture_moments(S, 1.0, E, c, vc), "moments")
        st, want_st = {}, {}
        want = ref.denoise_moments(S, planes, w, rows, 1.0, E, c, vc, stats=want_st, **opts)
        same(capi.history_denoise_moments_counted_host(S, planes, w, rows, 1.0, E, c, vc, stats=st, **opts), want, "filter")
        same(st["var_raw"], want_st["var_raw"])
        assert np.array_equal(st["mark"], want_st["mark"])
    if n > 100:
        K = capi.history_capture_counted_host(S, planes, 1.0, E, C)
        assert (K[0, :, 3] == f32(1.0) + E + C[:, 3]).all() and (E > 0).any() and (E == 0).any()
        assert not np.array_equal(bits(capi.history_blend_counted_host(S, 1.0, E, C)), bits(capi.history_blend_host(S, 1.0, C)))


def test_host_refusals():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, rows = 5, 3
    n, S, planes, C, VC = frame(w, rows)
    feat, cur = ref.random_planes(w, rows)
    E = np.zeros(n, f32)
    lib = capi.lib()

    def refused(call, *phrases):
        with pytest.raises(capi.PtError) as e:
            call()
        for p in phrases:
            assert p in str(e.value), (p, str(e.value))

    who = "pt_history_select_host"
    refused(lambda: capi.history_select_host(feat, w, rows, cur, ref.EMITTER, min_history=float("nan")), who, "finite")
    refused(lambda: capi.history_select_host(feat, w, rows, cur, ref.EMITTER, min_history=float("inf")), who, "finite")
    refused(lambda: capi.history_select_host(feat, w, rows, cur, ref.EMITTER, min_history=-1.0), who, "min_history")
    refused(lambda: capi.history_select_host(feat, w, rows, cur, ref.EMITTER, max_fraction=-0.5), who, "max_fraction")
    refused(lambda: capi.history_select_host(feat, w, rows, cur, ref.EMITTER, max_fraction=1.5), who, "max_fraction")
    one = np.zeros(1, np.int32)
    a, b = capi.C.c_int32(), capi.C.c_int32()
    assert lib.pt_history_select_host(0, rows, capi._f(feat.reshape(-1)), None, None, 0, None, capi._i(one), capi.C.byref(a), capi.C.byref(b)) != 0
    assert who in lib.pt_last_error().decode() and "not supported" in lib.pt_last_error().decode()
    assert lib.pt_history_select_host(w, rows, capi._f(feat.reshape(-1)), None, None, 3, None, capi._i(one), capi.C.byref(a), capi.C.byref(b)) != 0
    assert "emitter_geom" in lib.pt_last_error().decode()
    assert lib.pt_history_select_host(w, rows, None, None, None, 0, None, capi._i(one), capi.C.byref(a), capi.C.byref(b)) != 0
    assert "null" in lib.pt_last_error().decode()

    who = "pt_history_merge_host"
    Sw = ref.random_image(2)
    refused(lambda: capi.history_merge_host(S, E, [3, 3], Sw, 4), who, "repeated")
    refused(lambda: capi.history_merge_host(S, E, [3, n], Sw, 4), who, "outside")
    refused(lambda: capi.history_merge_host(S, E, [-1, 2], Sw, 4), who, "outside")
    refused(lambda: capi.history_merge_host(S, E, [1, 2], Sw, 0), who, "group of 0")
    refused(lambda: capi.history_merge_host(S, E, np.zeros(0, np.int32), np.zeros((0, 3), f32), 4), who, "list of 0")

    bad = E.copy()
    bad[4] = -1.0
    nan = E.copy()
    nan[2] = np.nan
    for name, call in (("pt_history_blend_counted_host", lambda s, e, c=C, v=VC: capi.history_blend_counted_host(S, s, e, c)),
                       ("pt_history_capture_counted_host", lambda s, e, c=C, v=VC: capi.history_capture_counted_host(S, planes, s, e, c)),
                       ("pt_history_capture_moments_counted_host", lambda s, e, c=C, v=VC: capi.history_capture_moments_counted_host(S, s, e, c, v)),
                       ("pt_history_denoise_moments_counted_host",
                        lambda s, e, c=C, v=VC: capi.history_denoise_moments_counted_host(S, planes, w, rows, s, e, c, v))):
        for samples in (0.0, -1.0, float("nan"), float("inf")):
            refused(lambda: call(samples, E), name, "samples")
        refused(lambda: call(1.0, bad), name, "extra[4]")
        refused(lambda: call(1.0, nan), name, "extra[2]")
        call(1.0, E)
    refused(lambda: capi.history_capture_moments_counted_host(S, 1.0, E, C, None), "pt_history_capture_moments_counted_host", "moments")
    refused(lambda: capi.history_denoise_moments_counted_host(S, planes, w, rows, 1.0, E, C, None), "pt_history_denoise_moments_counted_host", "moments")
    refused(lambda: capi.history_denoise_moments_counted_host(S, planes, w, rows, 1.0, E, C, VC, levels=9), "pt_history_denoise_moments_counted_host", "levels")


@pytest.mark.parametrize("w,rows", [(5, 3), (97, 61)])
def test_host_code_under_the_sanitizers(tmp_path, w, rows):
    """pt_history.h and pt_denoise.h are plain C++: a stand-alone driver (tests/integration/history_round_driver.cpp) runs the key, the
    selection, the merge and the counted forms with address and undefined-behaviour checks, built by the system compiler and run directly."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no system C++ compiler on this machine")
    exe = str(tmp_path / "history_round_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
           "-I", CSRC, os.path.join(ROOT, "tests", "integration", "history_round_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(w), str(rows)], capture_output=True, text=True)
    assert r.returncode == 0 and "selected" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)
    selected = int(r.stdout.split(":")[1].split()[0])
    assert 0 < selected < w * rows
