"""The history probes on the host (no GPU): pt_history_probe_list_host, _keep_host, _gradient_host and _apply_host against
tests/history_probe_ref.py, bit for bit; their refusals; and the host loops under the sanitizers in a stand-alone program
(tests/integration/history_probe_driver.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import history_probe_ref as ref
from history_probe_ref import bits, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "csrc")
PHASES = range(9)


def same(got, want, what=""):
    assert np.array_equal(bits(got), bits(want)), what


@pytest.mark.parametrize("w,rows", ref.SHAPES)
def test_list_equals_the_restatement(w, rows):
    """All nine phases, those with PW or PR = 0 included: every probe a tile pixel at (3 i + ox, 3 j + oy), ascending, and together the
    nine phases list every pixel once."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    seen = np.zeros(w * rows, np.int32)
    for phase in PHASES:
        lst = capi.history_probe_list_host(w, rows, phase)
        assert np.array_equal(lst, ref.probe_list(w, rows, phase)), phase
        ox, oy, PW, PR = ref.grid(w, rows, phase)
        assert lst.size == PW * PR
        assert PW == (0 if w <= ox else (w - ox + 2) // 3) and PR == (0 if rows <= oy else (rows - oy + 2) // 3)
        assert (np.diff(lst) > 0).all() and ((lst % w) % 3 == ox).all() and ((lst // w) % 3 == oy).all()
        seen[lst] += 1
    assert (seen == 1).all()
    if w < 3 or rows < 3:
        assert any(ref.probe_list(w, rows, p).size == 0 for p in PHASES)


@pytest.mark.parametrize("w,rows", ref.SHAPES)
def test_keep_and_gradient_equal_the_restatement(w, rows):
    """lam exactly 0, above 1 (clamped), m == 0, infinite and NaN sums (read as 1); skipped: another id, a miss, an id outside the table,
    a moved geom."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    kinds = set()
    for phase in PHASES:
        S, feat, PK, Sw, _ = ref.random_case(w, rows, phase)
        same(capi.history_probe_keep_host(S, feat, w, rows, phase), ref.keep(S, feat, w, rows, phase), f"keep, phase {phase}")
        for moved in (ref.MOVED, np.zeros(ref.NUM_GEOMS, np.uint8), ()):
            L, changed, skipped = capi.history_probe_gradient_host(PK, Sw, feat, w, rows, phase, moved)
            want, want_changed, want_skipped = ref.gradient(PK, Sw, feat, w, rows, phase, moved)
            same(L, want, f"L, phase {phase}")
            assert (changed, skipped) == (want_changed, want_skipped) == (int((L > 0).sum()), int((L < 0).sum()))
            assert ((L == -1) | ((L >= 0) & (L <= 1))).all()
            if len(moved) == 0:
                assert skipped == L.size  # no geom table: every id lies outside it
        L, _, _ = capi.history_probe_gradient_host(PK, Sw, feat, w, rows, phase, ref.MOVED)
        lst = ref.probe_list(w, rows, phase)
        ids, kept_ids = ref.ids_of(feat)[lst], np.ascontiguousarray(PK[:, 3]).view(np.int32)
        live = L >= 0
        if live.any():
            assert (ids[live] == kept_ids[live]).all() and (ref.MOVED[ids[live] - 1] == 0).all()
        bad = ~np.isfinite(Sw).all(axis=1) | ~np.isfinite(PK[:, :3]).all(axis=1)
        assert (L[live & bad] == 1).all()
        both_zero = (PK[:, :3] == 0).all(axis=1) & (Sw == 0).all(axis=1)
        assert (bits(L[live & both_zero]) == 0).all()
        equal = (bits(PK[:, :3]) == bits(Sw)).all(axis=1) & ~bad
        assert (bits(L[live & equal]) == 0).all()
        kinds |= {"zero"} if (live & equal).any() else set()
        kinds |= {"one"} if (L == 1).any() else set()
        kinds |= {"between"} if ((L > 0) & (L < 1)).any() else set()
        kinds |= {"nonfinite"} if (live & bad).any() else set()
        kinds |= {"m0"} if (live & both_zero).any() else set()
        kinds |= {"other id"} if (ids != kept_ids).any() else set()
        kinds |= {"miss"} if (ids == 0).any() else set()
        kinds |= {"moved"} if ((ids >= 1) & (ids <= ref.NUM_GEOMS) & (ids == kept_ids) & (L < 0)).any() else set()
    if w * rows > 1000:
        assert kinds == {"zero", "one", "between", "nonfinite", "m0", "other id", "miss", "moved"}, kinds


@pytest.mark.parametrize("w,rows", ref.SHAPES)
def test_apply_equals_the_restatement(w, rows):
    """Radius 0 .. 4, gain below and above 1; misses, ids outside the table and pixels of moved geoms keep every word, and so does every
    pixel whose lam_p is 0 — its -0 and NaN words included; nothing but C.w is ever written."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    for phase in PHASES:
        S, feat, PK, Sw, C = ref.random_case(w, rows, phase, seed=1)
        L, _, _ = ref.gradient(PK, Sw, feat, w, rows, phase, ref.MOVED)
        for radius, gain in ((0, 0.0), (-1, 0.0), (1, 0.5), (2, 3.0), (3, 1.0), (4, 0.25)):
            got = capi.history_probe_apply_host(C, L, feat, w, rows, phase, ref.MOVED, radius, gain)
            same(got, ref.apply(C, L, feat, w, rows, phase, ref.MOVED, radius, gain), f"phase {phase}, radius {radius}, gain {gain}")
            r = ref.RADIUS if radius == 0 else 0 if radius == -1 else radius
            lam = np.where(ref.eligible(feat, ref.MOVED), ref.lam_pixels(L, w, rows, phase, r), 0)
            keepers = lam == 0
            same(got[keepers], C[keepers], "a pixel with lam_p == 0 changed")
            same(got[:, :3], C[:, :3], "a word other than C.w changed")
            full = (lam * f32(gain or ref.GAIN) >= 1) & np.isfinite(C[:, 3])
            assert (got[full, 3] == 0).all()
        if w * rows > 1000 and phase == 4:
            lam = np.where(ref.eligible(feat, ref.MOVED), ref.lam_pixels(L, w, rows, phase, ref.RADIUS), 0)
            w_bits = bits(C[:, 3])
            assert ((lam == 0) & (w_bits == 0x80000000)).any() and ((lam == 0) & np.isnan(C[:, 3])).any()
            assert (~ref.eligible(feat, ref.MOVED) & (ref.lam_pixels(L, w, rows, phase, ref.RADIUS) > 0)).any()  # an excluded pixel beside a changed probe
            assert (lam > 0).any() and (lam == 0).any()
    # skipped probes add nothing: with every probe skipped no pixel changes
    S, feat, PK, Sw, C = ref.random_case(w, rows, 0, seed=2)
    L = np.full(ref.probe_list(w, rows, 0).size, -1, f32)
    same(capi.history_probe_apply_host(C, L, feat, w, rows, 0, ref.MOVED, 4, 8.0), C)


def test_host_refusals():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, rows = 7, 3
    S, feat, PK, Sw, C = ref.random_case(w, rows, 0)
    L, _, _ = ref.gradient(PK, Sw, feat, w, rows, 0, ref.MOVED)

    def refused(call, *phrases):
        with pytest.raises(capi.PtError) as e:
            call()
        for p in phrases:
            assert p in str(e.value), (p, str(e.value))

    for phase in (-1, 9):
        refused(lambda: capi.history_probe_list_host(w, rows, phase), "pt_history_probe_list_host", "phase")
    refused(lambda: capi.history_probe_list_host(0, rows, 0), "pt_history_probe_list_host", "not supported")
    who = "pt_history_probe_apply_host"
    for radius in (5, -2):
        refused(lambda: capi.history_probe_apply_host(C, L, feat, w, rows, 0, ref.MOVED, radius), who, "radius")
    refused(lambda: capi.history_probe_apply_host(C, L, feat, w, rows, 0, ref.MOVED, 1, -1.0), who, "gain")
    for gain in (float("nan"), float("inf")):
        refused(lambda: capi.history_probe_apply_host(C, L, feat, w, rows, 0, ref.MOVED, 1, gain), who, "finite")
    lib = capi.lib()
    lam = np.zeros(L.size, f32)
    assert lib.pt_history_probe_gradient_host(w, rows, 0, capi._f(PK.reshape(-1)), capi._f(Sw.reshape(-1)), capi._f(feat.reshape(-1)), None, 3, capi._f(lam),
                                              None, None) != 0
    assert "moved_geom" in lib.pt_last_error().decode()
    assert lib.pt_history_probe_keep_host(w, rows, 0, None, capi._f(feat.reshape(-1)), capi._f(lam)) != 0
    assert "pt_history_probe_keep_host" in lib.pt_last_error().decode() and "null" in lib.pt_last_error().decode()


@pytest.mark.parametrize("w,rows", [(1, 1), (4, 5), (97, 61)])
def test_host_code_under_the_sanitizers(tmp_path, w, rows):
    """pt_history.h is plain C++: a stand-alone driver (tests/integration/history_probe_driver.cpp) runs the list, the keep, the gradient
    and the apply at all nine phases and radius 0 .. 4 with address and undefined-behaviour checks, built by the system compiler and run
    directly."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no system C++ compiler on this machine")
    exe = str(tmp_path / "history_probe_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
           "-I", CSRC, os.path.join(ROOT, "tests", "integration", "history_probe_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(w), str(rows)], capture_output=True, text=True)
    assert r.returncode == 0 and "changed" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)
    if w * rows > 100:
        changed = int(r.stdout.split("changed:")[1].split()[0])
        assert changed > 0
