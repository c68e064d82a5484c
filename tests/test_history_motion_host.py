"""The objects' motion on the host: pt_scene_set_geom_trs against scene files, pt_history_motion_host and
pt_history_reproject_motion_host (csrc/pt_history.h, the bodies the HIP kernel runs too) against the numpy restatement
tests/history_motion_ref.py, bit for bit, and a geometric property that needs no reference.  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import history_moments_ref as mref
import history_motion_ref as ref
import history_ref as href
import history_variance_ref as vref
from history_ref import bits, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "csrc")


def same(got, want, what=""):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


def matrices(g):
    return np.array(list(g.transform) + list(g.inverseTransform) + list(g.invTranspose), f32).view(np.uint32)


# ---- pt_scene_set_geom_trs ------------------------------------------------------------------------------------------------------
# binary-exact values: the text of the file and the float32 the setter takes are the same numbers
MOVES = {6: (-2.5, 4.25, -1.0, 0.0, 0.0, 0.0, 3.0, 3.0, 3.0),        # the sphere, translated
         4: (-4.5, 5.0, 0.5, 22.5, 45.0, 11.25, 0.125, 8.0, 9.5)}   # the left wall: a rotated, scaled cube


@pytest.mark.parametrize("geom", sorted(MOVES))
def test_set_geom_trs_gives_the_loaders_matrices(tmp_path, geom):
    from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes
    trs = MOVES[geom]
    home = capi.Scene(scenes.write_scene(scenes.cornell_scene_text(res=(96, 54)), str(tmp_path / "home.txt")))
    moved_text = scenes.cornell_scene_text(res=(96, 54), objects={geom: dict(trans=trs[0:3], rotat=trs[3:6], scale=trs[6:9])})
    there = capi.Scene(scenes.write_scene(moved_text, str(tmp_path / "there.txt")))
    before = [matrices(g).copy() for g in home.geoms()]
    assert not np.array_equal(before[geom], matrices(there.geoms()[geom]))
    home.set_geom_trs(geom, trs)
    for i, (a, b) in enumerate(zip(home.geoms(), there.geoms())):
        assert np.array_equal(matrices(a), matrices(b)), i
        assert (a.type, a.materialid) == (b.type, b.materialid)
        if i != geom:
            assert np.array_equal(matrices(a), before[i]), i
    same(home.geom_trs(geom), np.array(trs, f32))
    same(home.geom_trs(0), np.array((0, 10, 0, 0, 0, 0, 3, 0.3, 3), f32))  # cornell.txt's light, as the loader read it


def test_cornell_text_default_is_unchanged():
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    assert scenes.cornell_scene_text() == scenes.cornell_scene_text(objects={})
    assert scenes.cornell_scene_text(objects={6: dict(trans=(-1, 4, -1))}) == scenes.cornell_scene_text()
    assert "TRANS       -2.5 4 -1" in scenes.cornell_scene_text(objects=ref.sphere_objects(0))


def test_set_geom_trs_refusals(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes
    sc = capi.Scene(scenes.write_scene(scenes.mesh_scene_text(), str(tmp_path / "mesh.txt")))
    n = sc.desc.num_geoms
    tri = next(i for i, g in enumerate(sc.geoms()) if g.type == 2)
    ok = (0, 0, 0, 0, 0, 0, 1, 1, 1)
    for who, call in (("pt_scene_set_geom_trs", lambda g, t: sc.set_geom_trs(g, t)), ("pt_scene_geom_trs", lambda g, t: sc.geom_trs(g))):
        for g, phrase in ((-1, "outside"), (n, "outside"), (tri, "mesh")):
            with pytest.raises(capi.PtError, match=who + ".*" + phrase):
                call(g, ok)
    with pytest.raises(capi.PtError, match=r"pt_scene_set_geom_trs: trs\[4\] is not finite"):
        sc.set_geom_trs(0, (0, 0, 0, 0, float("nan"), 0, 1, 1, 1))
    assert capi.lib().pt_scene_set_geom_trs(None, 0, None) != 0


# ---- pt_history_motion_host -----------------------------------------------------------------------------------------------------
def test_motion_table_against_float64():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    kept, cur = ref.mixed_geoms()
    table, kind = capi.history_motion_host(kept, cur)
    want_table, want_kind = ref.motion_table(kept, cur)
    assert list(kind) == list(want_kind) == [ref.STILL, ref.MOVED, ref.MOVED, ref.NOTHING, ref.NOTHING, ref.STILL]
    same(table, want_table)
    assert not np.isfinite(table[4, :21]).all()                      # the singular transform
    assert (table[:, 21:] == 0).all()
    # a pure translation: D = identity | kept - current, Nm = identity
    same(table[1, :12], np.array([1, 0, 0, -0.5, 0, 1, 0, 0, 0, 0, 1, 0.25], f32))
    same(table[1, 12:21], np.eye(3, dtype=f32).ravel())
    # the table takes a point of the current object to where it was: transform_kept (inverse_current p)
    D = table[2, :12].reshape(3, 4).astype(np.float64)
    A_k, B_c = (np.array(list(m), np.float64).reshape(4, 4).T for m in (kept[2].transform, cur[2].inverseTransform))
    p = np.array([0.3, -0.2, 0.9, 1.0])
    assert np.allclose(D @ p, (A_k @ (B_c @ p))[:3], rtol=1e-5, atol=1e-5)
    # ... and the other way round it is the inverse, to float32
    back, _ = capi.history_motion_host(cur, kept)
    M = np.vstack([table[2, :12].reshape(3, 4), [0, 0, 0, 1]]).astype(np.float64) @ np.vstack([back[2, :12].reshape(3, 4), [0, 0, 0, 1]]).astype(np.float64)
    assert np.allclose(M, np.eye(4), atol=1e-5)


def test_motion_table_refusals():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    L = capi.lib()
    assert L.pt_history_motion_host(None, None, 1, None, None) != 0
    assert "pt_history_motion_host" in L.pt_last_error().decode()


# ---- pt_history_reproject_motion_host -------------------------------------------------------------------------------------------
def run_host(capi, cam, kept, feat, reject, table, kind, vk, w, rows, row0, flags, **opts):
    return capi.history_reproject_motion_host(cam.to_capi(), kept, feat, reject, table, kind, w, rows, row0, flags=flags,
                                              kept_var=vk if flags & 3 else None, **opts)


@pytest.mark.parametrize("name", sorted(href.OPTION_SETS))
@pytest.mark.parametrize("kind_name", sorted(ref.KINDS))
@pytest.mark.parametrize("row0", href.ROW0)
@pytest.mark.parametrize("w,rows", href.SHAPES)
def test_lookup_with_motion_on_adversarial_arrays(w, rows, row0, kind_name, name):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    cam, kept, feat, reject, _, table, kind, vk = ref.adversarial(w, rows, row0)
    flags, opts = ref.KINDS[kind_name], href.OPTION_SETS[name]
    got = run_host(capi, cam, kept, feat, reject, table, kind, vk, w, rows, row0, flags, **opts)
    stats = {}
    want = ref.reproject_motion(cam, kept, feat, reject, table, kind, w, rows, row0, flags=flags, kept_var=vk, stats=stats, **opts)
    if flags & 3:
        same(got[0], want[0], "C"), same(got[1], want[1], "VC")
        same(got[0], ref.reproject_motion(cam, kept, feat, reject, table, kind, w, rows, row0, **opts), "C does not depend on the kind")
        C = got[0]
    else:
        same(got, want, "C")
        C = got
    if w * rows > 1000:  # the large shape exercises every branch: moved pixels that carry, kind-2 pixels that do not
        ids = href.surface(feat)[3]
        assert stats["moved"].sum() > 100 and (C[stats["moved"], 3] > 0).sum() > 20
        assert (C[ids == 4] == 0).all() and (C[(ids == 1) | (ids == 6), 3] > 0).sum() > 20
        if not opts.get("keep_view_dependent"):
            assert (C[ids == 3] == 0).all()  # the mirror: rejected before the motion step
        else:
            assert (C[ids == 3, 3] > 0).any()


@pytest.mark.parametrize("w,rows,row0", [(5, 3, 0), (97, 61, 7)])
def test_every_geom_still_is_the_flagless_lookup(w, rows, row0):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    cam, kept, feat, reject, _, table, _, vk = ref.adversarial(w, rows, row0)
    still = np.zeros(href.NUM_GEOMS, np.uint8)
    for name, opts in href.OPTION_SETS.items():
        c = cam.to_capi()
        same(run_host(capi, cam, kept, feat, reject, table, still, vk, w, rows, row0, ref.MOTION, **opts),
             capi.history_reproject_host(c, kept, feat, reject, w, rows, row0, **opts), name)
        for flags, plain in ((ref.VARIANCE, capi.history_reproject_variance_host), (ref.MOMENTS, capi.history_reproject_moments_host)):
            got = run_host(capi, cam, kept, feat, reject, table, still, vk, w, rows, row0, ref.MOTION | flags, **opts)
            want = plain(c, kept, feat, reject, vk, w, rows, row0, **opts)
            same(got[0], want[0], name), same(got[1], want[1], name)
    # ... and the numpy restatements agree with each other
    same(ref.reproject_motion(cam, kept, feat, reject, table, still, w, rows, row0), href.reproject(cam, kept, feat, reject, w, rows, row0))
    got = ref.reproject_motion(cam, kept, feat, reject, table, still, w, rows, row0, flags=ref.MOTION | ref.VARIANCE, kept_var=vk)
    want = vref.reproject_variance(cam, kept, feat, reject, vk, w, rows, row0)
    same(got[0], want[0]), same(got[1], want[1])
    got = ref.reproject_motion(cam, kept, feat, reject, table, still, w, rows, row0, flags=ref.MOTION | ref.MOMENTS, kept_var=vk)
    want = mref.reproject_moments(cam, kept, feat, reject, vk, w, rows, row0)
    same(got[0], want[0]), same(got[1], want[1])


def test_lookup_with_motion_refusals():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, rows = 5, 3
    cam, kept, feat, reject, _, table, kind, vk = ref.adversarial(w, rows, 0)
    who = "pt_history_reproject_motion_host"

    def refused(flags, phrase, kind=kind, vk=vk):
        with pytest.raises(capi.PtError, match=who + ".*" + phrase):
            capi.history_reproject_motion_host(cam.to_capi(), kept, feat, reject, table, kind, w, rows, 0, flags=flags, kept_var=vk)

    refused(8 | ref.MOTION, "undefined flag")
    refused(ref.MOTION | 3, "exclude each other")
    refused(ref.MOTION, "kind", kind=np.array([0, 1, 3, 0, 0, 0], np.uint8))
    refused(ref.MOTION | ref.MOMENTS, "null", vk=None)


# ---- a property that needs no reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, -2])
def test_a_translated_plane_carries_its_ramp_with_it(k):
    """A camera-facing plane of one geom whose kept colour is a linear ramp in x; the geom moves by exactly k pixels' worth along the
    camera's -right axis.  The motion lookup returns the ramp shifted by k; the plain lookup on the same input the unshifted ramp."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, rows, depth, slope = 97, 61, 8.0, 0.25
    cam = href.Cam(w, rows)
    n = w * rows
    xs, ys = np.meshgrid(np.arange(w), np.arange(rows))
    xs, ys = xs.ravel(), ys.ravel()
    pts = np.array([href.point_at(cam, float(x), float(y), depth) for x, y in zip(xs, ys)], f32)  # pixel x looks along sx = x
    kept = np.zeros((3, n, 4), f32)
    kept[0, :, 0], kept[0, :, 1], kept[0, :, 2], kept[0, :, 3] = slope * xs, 1.0, 0.5, 4.0
    kept[1, :, :3], kept[1, :, 3] = pts, np.ones(n, np.int32).view(f32)
    kept[2, :, 2] = -1.0
    # the current view: the same pixels see the plane's points, which moved with the geom: pixel x now sees what pixel x - k saw
    step = k * depth * cam.pixelLength[0]  # k pixels' worth at this depth, along +x (the camera's right is -x: screen x grows with world x)
    feat = np.zeros((3, n, 4), f32)
    feat[0, :, 2], feat[1, :, :3], feat[1, :, 3] = -1.0, 0.5, 1.0
    feat[2, :, :3], feat[2, :, 3] = pts, kept[1, :, 3]
    g_kept, g_cur = ref.geom((0, 0, 2, 0, 0, 0, 40, 40, 0.5)), ref.geom((step, 0, 2, 0, 0, 0, 40, 40, 0.5))
    table, kind = capi.history_motion_host([g_kept], [g_cur])
    assert list(kind) == [ref.MOVED]
    reject = np.zeros(1, np.uint8)
    C = capi.history_reproject_motion_host(cam.to_capi(), kept, feat, reject, table, kind, w, rows).reshape(rows, w, 4)
    plain = capi.history_reproject_host(cam.to_capi(), kept, feat, reject, w, rows).reshape(rows, w, 4)
    x = np.arange(w)
    interior = (x - k >= 1) & (x - k <= w - 2)
    assert (C[1:-1, interior, 3] > 0).all()
    # the ramp's slope times 1e-3 pixel (float32 coordinate rounding at W = 97 is below 1e-4 pixel)
    assert np.abs(C[1:-1, interior, 0] - slope * (x[interior] - k)).max() <= slope * 1e-3
    assert np.abs(plain[1:-1, 1:-1, 0] - slope * x[1:-1]).max() <= slope * 1e-3
    same(C[1:-1, interior, 1:3], np.broadcast_to(np.array([1.0, 0.5], f32), C[1:-1, interior, 1:3].shape))


# ---- the sanitizers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,rows", [(1, 1), (5, 3), (97, 61)])
def test_host_code_under_the_sanitizers(tmp_path, w, rows):
    """pt_history.h is plain C++: a stand-alone driver (tests/integration/history_motion_driver.cpp) builds the motion table and runs
    the lookup in its three kinds with address and undefined-behaviour checks, built by the system compiler and run directly."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no system C++ compiler on this machine")
    exe = str(tmp_path / "history_motion_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
           "-I", CSRC, os.path.join(ROOT, "tests", "integration", "history_motion_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(w), str(rows)], capture_output=True, text=True)
    assert r.returncode == 0 and "carried" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)
    still, moved, tri = ((int(a), int(b)) for a, b in re.findall(r"(\d+) of (\d+)", r.stdout))
    own = int(re.search(r"\((\d+) on their own", r.stdout).group(1))
    assert still[0] == still[1] and moved[0] == moved[1] == own and tri[0] == 0
    assert sum(p[1] for p in (still, moved, tri)) == w * rows - (1 if w * rows > 4 else 0)  # every pixel but the miss
