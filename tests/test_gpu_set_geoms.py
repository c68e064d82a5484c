"""Moving the objects of a live renderer (pt_set_geoms): after the call the renderer gives what a renderer freshly created from the
scene with those geoms gives, bit for bit — image, feature planes, noise planes, a threshold round, the tables on the device — with
the tree, the top list, the grid and the batch buffers of the previous geoms gone.  The moved scenes are scene files (cornell:
scenes.cornell_scene_text(objects=...)) or Scene.set_geom_trs on a loaded scene, which tests/test_history_motion_host.py shows to be
the same bytes."""
import ctypes as C

import numpy as np
import pytest

import history_motion_ref as mref
from camera_scenes import cornell_text, random_text, scene_path, stress_text
from cosc_4397_pathtracing_raytracing_project_amd import scenes

pytestmark = pytest.mark.gpu
f32 = np.float32
THRESHOLD, FRACTION = 0.02, 0.25


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def render_two_calls(r):
    r.render(1, 3)
    r.render(4, 5)
    return r.readback()


def sphere_path(tmp_path, x):
    return scenes.write_scene(cornell_text(objects={6: dict(trans=(x, 4, -1))}), str(tmp_path / f"cornell_sphere_{x}.txt"))


# ---- cornell, every arithmetic mode, against a fresh renderer and the oracle ----------------------------------------------------
@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
def test_cornell_sphere_moved_equals_fresh_and_oracle(tmp_path, oracle, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    xs = (-1, -2.5, 0.5, 3.25)  # -1: cornell.txt's own
    paths = {x: sphere_path(tmp_path, x) for x in xs}
    want = {}
    for x in xs:
        r = capi.Renderer(capi.Scene(paths[x]), arith=arith)
        try:
            want[x] = render_two_calls(r)
        finally:
            r.free()
    assert len({bits(want[x]).tobytes() for x in xs}) == len(xs)
    r = capi.Renderer(capi.Scene(paths[-1]), arith=arith)
    try:
        assert np.array_equal(bits(render_two_calls(r)), bits(want[-1]))
        for x in xs[1:] + xs[:1]:
            r.set_geoms(capi.Scene(paths[x]))
            assert not r.readback().any() and r.stats().samples == 0  # everything pt_clear does
            got = render_two_calls(r)
            bad = np.flatnonzero((bits(got) != bits(want[x])).any(axis=1))
            assert bad.size == 0, (arith, x, bad.size, bad[:4], got[bad[:2]], want[x][bad[:2]])
            if arith == "exact":
                oracle.set_math_mode(oracle.PORTABLE)
                oracle.load_scene(paths[x])
                ref = oracle.render(1, 8, depth=8, variant=oracle.RETIRE, nthreads=16)
                assert np.array_equal(bits(got), bits(ref)), x
        t = r.set_geoms_times()
        assert t.total_ms > 0 and t.build_ms > 0 and t.upload_ms > 0 and t.rearm_ms > 0 and t.total_ms >= t.build_ms + t.upload_ms
        assert r.setup_times().set_camera_calls == 0  # pt_get_setup_times gains nothing
    finally:
        r.free()


# ---- scenes with tightened leaves and a grid: the tree's shape, the bounds and the tables follow the geoms ---------------------------
def sequence(r):
    """render, features, two folds, one threshold round, then what can be read, the tables on the device among it."""
    out = {}
    r.render(1, 4)
    r.render_features(1, 4)
    r.noise_fold()
    r.render(5, 4)
    r.noise_fold()
    out["round"] = r.adaptive_round_threshold(9, 4, THRESHOLD, FRACTION)
    out["image"] = r.readback()
    for k, v in r.readback_noise().items():
        out["noise_" + k] = v
    for k, v in r.readback_features().items():
        out["feature_" + k] = v
    out["counts"] = r.readback_adaptive()
    st = r.stats()
    out["tight_leaves"] = st.tight_leaves
    tables = r.read_tables()
    grid = tuple(r.grid_info()[0].res) if st.grid_cells else None
    return out, tables, grid


def same(a, b):
    if isinstance(a, np.ndarray):
        return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    return a == b


def moves_of(scene):
    """(name, geom, trs) of the three moves: one object far outside the scene's bounds; the object furthest to the left carried across
    all its neighbours to the right (the tree's median splits change); the same geoms again."""
    n = scene.desc.num_geoms
    free = range(6, n)  # behind cornell's walls and light
    trs = {g: scene.geom_trs(g) for g in free}
    out = trs[6].copy()
    out[:3] = (40.0, 5.0, -30.0)
    left = min(free, key=lambda g: trs[g][0])
    across = trs[left].copy()
    across[0] = max(t[0] for t in trs.values()) + 0.5
    return [("outside", 6, out), ("across", left, across), ("again", left, across)]


def tree_shape(scene):
    return [(nd.left, nd.right, nd.geomIndex) for nd in scene.bvh()]


@pytest.mark.parametrize("arith", ["exact", "fast"])
@pytest.mark.parametrize("text_fn,flags", [(random_text, 0), (random_text, 256), (stress_text, 256)])
def test_tables_follow_the_geoms(tmp_path, text_fn, flags, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path = scene_path(tmp_path, text_fn, "A")
    home = capi.Scene(path)
    shapes, bounds = {"home": tree_shape(home)}, {"home": list(home.bvh()[0].bmin) + list(home.bvh()[0].bmax)}
    moves = moves_of(home)
    # fresh renderers first (capi.Renderer is the default instance: a new one replaces the old), one per state; the moves accumulate
    want = {}
    moved = capi.Scene(path)
    for name, geom, trs in moves:
        moved.set_geom_trs(geom, trs)
        shapes[name], bounds[name] = tree_shape(moved), list(moved.bvh()[0].bmin) + list(moved.bvh()[0].bmax)
        fresh = capi.Renderer(moved, debug_flags=flags, arith=arith)
        try:
            want[name] = sequence(fresh)
        finally:
            fresh.free()
    live_scene = capi.Scene(path)
    r = capi.Renderer(live_scene, debug_flags=flags, arith=arith)
    try:
        init_grid = sequence(r)[2]  # a worker, folds and counts exist: all of it is forgotten and follows
        assert (init_grid is not None) == bool(flags)
        for name, geom, trs in moves:
            live_scene.set_geom_trs(geom, trs)
            r.set_geoms(live_scene)
            assert r.noise() == dict(sse=-1.0, groups=0, iterations=0) and not r.readback_adaptive().any()
            got, got_tables, got_grid = sequence(r)
            wanted, want_tables, want_grid = want[name]
            for k in wanted:
                assert same(got[k], wanted[k]), (text_fn.__name__, flags, arith, name, k)
            for k in ("nodes", "nodes_b", "top", "top_b", "cull_margin", "geoms"):
                assert got_tables[k] == want_tables[k], (name, k, len(got_tables[k]), len(want_tables[k]))
            if got_grid is not None:
                assert got_grid == init_grid, name  # init's resolution is kept
            if got_grid == want_grid:  # ... and where a fresh renderer's cost model agrees with it, the grid is the same bytes
                for k in ("grid_start", "grid_items", "grid_items_b"):
                    assert got_tables[k] == want_tables[k], (name, k)
    finally:
        r.free()
    assert bounds["outside"] != bounds["home"]       # the first move took an object outside the old bounds
    assert shapes["across"] != shapes["outside"]     # the second changed the tree's shape
    assert shapes["again"] == shapes["across"] and bounds["again"] == bounds["across"]


def test_device_tables_after_set_geoms(tmp_path):
    """A device-path camera move after pt_set_geoms builds from the new geoms: the device copy of the camera-independent tables was
    dropped and is uploaded again."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    home, there = scene_path(tmp_path, random_text, "A"), scene_path(tmp_path, random_text, "B")
    name, geom, trs = moves_of(capi.Scene(home))[1]
    moved = capi.Scene(there)
    moved.set_geom_trs(geom, trs)
    fresh = capi.Renderer(moved, debug_flags=256, arith="fast")
    try:
        want, want_tables = render_two_calls(fresh), fresh.read_tables()
    finally:
        fresh.free()
    live = capi.Scene(home)
    r = capi.Renderer(live, debug_flags=256, arith="fast")
    try:
        r.set_camera(capi.Scene(there).camera, device_tables=True)  # the device copy of the home geoms exists
        render_two_calls(r)
        r.set_camera(live.camera, device_tables=True)
        live.set_geom_trs(geom, trs)
        r.set_geoms(live)
        r.set_camera(capi.Scene(there).camera, device_tables=True)
        assert r.set_camera_times().path == 1 and r.set_camera_times().fallback == 0
        assert np.array_equal(bits(render_two_calls(r)), bits(want))
        got_tables = r.read_tables()
        for k in ("nodes", "nodes_b", "top", "top_b", "cull_margin", "geoms"):
            assert got_tables[k] == want_tables[k], k
    finally:
        r.free()


def test_group_set_geoms_equals_one_renderer(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    xs = (-1, 2.5)
    paths = {x: sphere_path(tmp_path, x) for x in xs}
    r = capi.Renderer(capi.Scene(paths[-1]))
    try:
        r.render(1, 4)
        r.set_geoms(capi.Scene(paths[2.5]))
        r.render(1, 8)
        want = r.readback()
    finally:
        r.free()
    g = capi.Group(capi.Scene(paths[-1]), [0, 0], transport="copy")
    try:
        g.render(1, 4)
        before = g.gather()
        bad = mref.copy_geoms(capi.Scene(paths[2.5]))
        bad[3].materialid = 2
        with pytest.raises(capi.PtError, match=r"pt_group_set_geoms: geom 3 has type 1 and material 2.*only the transforms may change"):
            g.set_geoms(bad)
        assert np.array_equal(bits(g.gather()), bits(before))  # nothing was cleared in either context
        g.set_geoms(capi.Scene(paths[2.5]))
        assert not g.gather().any()
        g.render(1, 8)
        assert np.array_equal(bits(g.gather()), bits(want))
        for i in range(2):
            t = capi.PtSetGeomsTimes()
            capi._check(capi.lib().pt_ctx_get_set_geoms_times(g.context(i), C.byref(t)))
            assert t.total_ms > 0
    finally:
        g.free()


# ---- refusals: by phrase, in order, with nothing changed ------------------------------------------------------------------------
def test_refusals(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    L = capi.lib()
    scene = capi.Scene(sphere_path(tmp_path, -1))
    moved = capi.Scene(sphere_path(tmp_path, 2.5))
    capi.pt_free()
    for geoms in (None, moved.desc.geoms):  # no renderer comes before null geoms
        assert L.pt_set_geoms(geoms, 7) != 0
        assert b"pt_set_geoms: pt_init has not been called" in L.pt_last_error()
    assert L.pt_get_set_geoms_times(C.byref(capi.PtSetGeomsTimes())) != 0
    r = capi.Renderer(scene)
    try:
        want = render_two_calls(r)
        before, tables = r.stats().device_bytes, r.read_tables()

        def refused(geoms, n, phrase):
            assert L.pt_set_geoms(geoms, n) != 0
            msg = L.pt_last_error().decode()
            assert msg.startswith("pt_set_geoms: ") and phrase in msg, msg

        refused(None, 3, "null geoms")                       # before the count
        refused(moved.desc.geoms, 6, "6 geoms, but the renderer was created with 7")
        bad = mref.copy_geoms(moved)
        arr = lambda gs: (capi.PtGeom * len(gs))(*gs)
        bad[2].transform[5] = float("nan")                   # the count comes before the geoms, type and material before the matrices,
        bad[4].type = 0                                      # and the first geom that differs is named
        bad[5].materialid = 1
        refused(arr(bad), 6, "6 geoms")
        refused(arr(bad), 7, "geom 4 has type 0 and material 2, the renderer's has type 1 and material 2")
        bad[4].type = 1
        refused(arr(bad), 7, "geom 5 has type 1 and material 1, the renderer's has type 1 and material 3")
        bad[5].materialid = 3
        bad[6].invTranspose[15] = float("inf")
        refused(arr(bad), 7, "geom 2 has a matrix element that is not finite")
        bad[2].transform[5] = 1.0
        refused(arr(bad), 7, "geom 6 has a matrix element that is not finite")
        st = r.stats()
        assert st.device_bytes == before and st.samples == 96 * 54 * 8 and r.read_tables() == tables
        assert r.set_geoms_times().total_ms == 0
        assert np.array_equal(bits(r.readback()), bits(want))  # nothing was cleared
        r.clear()
        assert np.array_equal(bits(render_two_calls(r)), bits(want))  # and the sphere is where it was
    finally:
        r.free()
