"""The camera-dependent scene tables built on the device (pt_set_camera_ex with PT_SET_CAMERA_DEVICE_TABLES, csrc/pt_camera_tables.hip):
the functions of the shared header give the host's bits on the GPU, the tables a device-path move leaves are the host path's byte
for byte (all eight of pt_stage_read_tables), a long cell keeps threaded order, images and state after such a move are a fresh
renderer's, a group does the same, and what the device build declines runs on the host and says so.  Frames are 96 x 54 or 96 x 64."""
import ctypes as C

import numpy as np
import pytest

import grid_rays
from camera_scenes import cornell_text, random_text, scene_path, stress_text
from test_gpu_set_camera import adaptive_sequence, bits, fresh, grid_bytes, render_two_calls, same

pytestmark = pytest.mark.gpu
RANDOM_TIGHT = dict(A=22, B=21, C=0, D=0, E=23)


def stress_big_text(eye=None, **kw):  # 1006 primitives: the forced grid of the cost model has 12 x 13 x 12 cells, more than one workgroup scans (1024)
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    return scenes.stress_scene_text(grid=(10, 10, 10), res=(96, 54), eye=eye, **kw)


def times_of(r):
    t = r.set_camera_times()
    return t.path, t.fallback


# ---- 1. the shared header on the device against the host ------------------------------------------------------------------------
@pytest.mark.parametrize("kind, name", list(enumerate(["sqrt", "divide", "nextafterf", "center_half_box", "sphere_tight_box", "cell_range"])))
def test_shared_header_gives_the_hosts_bits_on_the_device(kind, name):
    """The edge list of the kind plus 1 << 16 pseudo-random operand sets: no result may differ in any bit.  A failure of sqrt or
    divide is to be fixed in csrc/pt_camera_tables.h (sqrt64 / div64), not here."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    assert capi.selfcheck_camera_math(kind, 1 << 16, seed=20240611) == 0, name


def test_selfcheck_refuses_bad_arguments():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = C.c_uint64(0)
    assert capi.lib().pt_selfcheck_camera_math(6, 1, 0, C.byref(n)) != 0 and b"pt_selfcheck_camera_math" in capi.lib().pt_last_error()
    assert capi.lib().pt_selfcheck_camera_math(0, 1, 0, None) != 0


# ---- 2. the tables, byte for byte ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["exact", "fast"])
@pytest.mark.parametrize("text_fn, flags", [(random_text, 0), (random_text, 256), (stress_text, 0), (stress_text, 256), (stress_big_text, 256)])
def test_device_tables_equal_host_tables(tmp_path, text_fn, flags, arith):
    """Per camera, in the order B, C, D, E, A: a host-path move, all eight tables; away and back on the device path, all eight again."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    cams = {n: capi.Scene(scene_path(tmp_path, text_fn, n)).camera for n in "ABCDE"}
    r = capi.Renderer(capi.Scene(scene_path(tmp_path, text_fn, "A")), debug_flags=flags, arith=arith)
    try:
        r.set_camera(cams["A"])  # (a grid that init's probe kept but does not walk goes with the first move, on either path)
        before, host_a = r.stats().device_bytes, r.read_tables()
        # the first device-path move keeps the camera-independent tables and the workspace on the device: counted from then on
        r.set_camera(cams["A"], device_tables=True)
        assert times_of(r) == (1, 0)
        assert r.read_tables() == host_a  # the same camera: the same tables
        base_bytes = r.stats().device_bytes - grid_bytes(r, arith)
        assert r.stats().device_bytes > before
        walks_grid = r.stats().grid_cells > 0
        if flags and text_fn is not random_text:  # (without the flag init's probe chooses the structure, and among finer grids too)
            assert r.stats().grid_cells == (12 * 13 * 12 if text_fn is stress_big_text else 5 ** 3)
        if text_fn is random_text:
            assert r.stats().grid_cells == (64 if flags else 0)
        for n in "BCDEA":
            away = cams["A" if n != "A" else "B"]
            r.set_camera(cams[n])
            assert times_of(r) == (0, 0)
            host, st_host = r.read_tables(), r.stats()
            info_host = r.grid_info() if st_host.grid_cells else None
            r.set_camera(away)
            r.set_camera(cams[n], device_tables=True)
            assert times_of(r) == (1, 0), n  # (at D the host scalars already say "no grid": still the device path)
            dev, st_dev = r.read_tables(), r.stats()
            for name in capi.TABLE_NAMES:
                assert len(dev[name]) == len(host[name]), (n, name, len(dev[name]), len(host[name]))
                if dev[name] != host[name]:
                    a, b = np.frombuffer(dev[name], np.uint32), np.frombuffer(host[name], np.uint32)
                    bad = np.flatnonzero(a != b)
                    raise AssertionError((text_fn.__name__, flags, arith, n, name, bad.size, bad[:8], a[bad[:8]], b[bad[:8]]))
            assert bool(host["nodes_b"]) == bool(host["top_b"]) == (arith == "fast")
            assert bool(host["grid_items_b"]) == (arith == "fast" and st_host.grid_cells > 0)
            assert (st_dev.tight_leaves, st_dev.grid_cells, st_dev.device_bytes) == (st_host.tight_leaves, st_host.grid_cells, st_host.device_bytes), n
            assert st_dev.device_bytes - grid_bytes(r, arith) == base_bytes, n  # memory moves by the grid's tables and nothing else
            if text_fn is random_text:
                assert st_dev.tight_leaves == RANDOM_TIGHT[n], n
                assert st_dev.grid_cells == (0 if not flags or n == "D" else 64), n
            if walks_grid:
                assert (st_dev.grid_cells == 0) == (n == "D"), n
            if info_host:  # the host copy of the cell table is fetched when first asked for
                info, longest = r.grid_info()
                assert (info.num_records, longest, tuple(info.res), info.pad) == (info_host[0].num_records, info_host[1], tuple(info_host[0].res), info_host[0].pad)
                assert len(dev["grid_items"]) == 32 * info.num_records
        assert r.setup_times().set_camera_calls == 17
    finally:
        r.free()


# ---- 3. order inside a long cell --------------------------------------------------------------------------------------------------
def test_a_long_cell_keeps_threaded_order(tmp_path):
    """330 tiny primitives in one cell: more than a wave and more than a workgroup of 256 take part in that cell's scatter."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes
    sc = capi.Scene(scenes.write_scene(grid_rays.scene_text("crowded", res=(96, 54)), str(tmp_path / "crowded.txt")))
    home, moved = sc.camera, sc.camera
    for a, d in enumerate((0.75, -0.5, 1.25)):
        moved.position[a] += d
    r = capi.Renderer(sc, debug_flags=256)
    try:
        r.set_camera(moved)
        host = r.read_tables()
        r.set_camera(home)
        r.set_camera(moved, device_tables=True)
        assert times_of(r) == (1, 0)
        dev = r.read_tables()
        assert dev["grid_items"] == host["grid_items"] and dev["grid_start"] == host["grid_start"] and dev["nodes"] == host["nodes"]
        info, longest = r.grid_info()
        assert longest >= grid_rays.CROWD["n"] > 256
        guard = info.res[0] * info.res[1] + info.res[0] + 2
        start = np.frombuffer(dev["grid_start"], np.uint32)[guard:guard + info.num_cells + 1].astype(np.int64)
        c = int(np.argmax(np.diff(start)))
        skip = np.frombuffer(dev["grid_items"], np.int32).reshape(-1, 8)[start[c]:start[c + 1], 6]
        assert skip.size == longest and (np.diff(skip) > 0).all()
    finally:
        r.free()


# ---- 4. images and state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text_fn, flags, arith", [(random_text, 256, "exact"), (random_text, 256, "fma"), (random_text, 256, "fast"),
                                                   (cornell_text, 0, "exact")])
def test_images_after_a_device_move_equal_a_fresh_renderer(tmp_path, text_fn, flags, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    paths = {n: scene_path(tmp_path, text_fn, n) for n in "ABE"}
    want = {n: fresh(paths[n], features=True, debug_flags=flags, arith=arith) for n in "BE"}  # (before `r`: one default renderer at a time)
    r = capi.Renderer(capi.Scene(paths["A"]), debug_flags=flags, arith=arith)
    try:
        render_two_calls(r)
        for n in "BE":
            want_img, st_fresh, want_feat = want[n]
            r.set_camera(capi.Scene(paths[n]).camera, device_tables=True)
            assert times_of(r) == (1, 0)
            got = render_two_calls(r)
            bad = np.flatnonzero((bits(got) != bits(want_img)).any(axis=1))
            assert bad.size == 0, (arith, n, bad.size, bad[:4])
            r.render_features(1, 8)
            feat = r.readback_features()
            for k in want_feat:
                assert np.array_equal(bits(feat[k]), bits(want_feat[k])), (arith, n, k)
            assert r.stats().tight_leaves == st_fresh.tight_leaves and r.stats().samples == st_fresh.samples == r.n * 8
    finally:
        r.free()


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_state_is_forgotten_and_the_worker_follows_a_device_move(tmp_path, arith):
    """test_gpu_set_camera.py's check of the host path, with the device path: threshold rounds with a worker that exists before the move."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    paths = {n: scene_path(tmp_path, cornell_text, n) for n in "AB"}
    control = capi.Renderer(capi.Scene(paths["B"]), arith=arith)
    try:
        want = adaptive_sequence(control)
    finally:
        control.free()
    assert all(0 < m <= above for above, m in want["rounds"])  # the rounds rendered something: the worker ran
    r = capi.Renderer(capi.Scene(paths["A"]), arith=arith)
    try:
        at_a = adaptive_sequence(r)
        assert not same(at_a["image"], want["image"])
        r.set_camera(capi.Scene(paths["B"]).camera, device_tables=True)
        assert times_of(r) == (1, 0)
        assert not r.readback().any() and r.stats().samples == 0
        assert r.noise() == dict(sse=-1.0, groups=0, iterations=0)
        assert not r.readback_adaptive().any()
        got = adaptive_sequence(r)
        for k in want:
            assert same(got[k], want[k]), (arith, k)
    finally:
        r.free()


# ---- 5. a group ---------------------------------------------------------------------------------------------------------------------
def test_group_device_move_equals_the_single_renderer(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    paths = {n: scene_path(tmp_path, random_text, n) for n in "AB"}
    want_img, _, want_feat = fresh(paths["B"], features=True, debug_flags=256, arith="fast")
    g = capi.Group(capi.Scene(paths["A"]), [0, 0], transport="copy", debug_flags=256, arith="fast")
    try:
        g.render(1, 2)
        g.set_camera(capi.Scene(paths["B"]).camera, device_tables=True)
        for i in range(2):
            t = capi.PtSetCameraTimes()
            assert capi.lib().pt_ctx_get_set_camera_times(g.context(i), C.byref(t)) == 0
            assert (t.path, t.fallback) == (1, 0) and t.total_ms > 0 and t.tables_ms > 0 and t.rearm_ms > 0
        g.render(1, 3)
        g.render(4, 5)
        assert np.array_equal(bits(g.gather()), bits(want_img))
        g.render_features(1, 8)
        feat = g.gather_features()
        for k in want_feat:
            assert np.array_equal(bits(feat[k]), bits(want_feat[k])), k
        bad = capi.Scene(paths["B"]).camera
        with pytest.raises(capi.PtError, match=r"pt_group_set_camera_ex: undefined flag bit\(s\) 0x6"):
            capi._check(capi.lib().pt_group_set_camera_ex(g._h, C.byref(bad), 7))
    finally:
        g.free()


# ---- 6. refusals, the plain form, the fallback ------------------------------------------------------------------------------------
def test_refusals_and_the_plain_form(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    L = capi.lib()
    paths = {n: scene_path(tmp_path, random_text, n) for n in "AB"}
    cam_b = capi.Scene(paths["B"]).camera
    capi.pt_free()
    for cam in (None, C.byref(cam_b)):  # no renderer comes first, whatever the flags
        assert L.pt_set_camera_ex(cam, 2) != 0 and b"pt_set_camera_ex: pt_init has not been called" in L.pt_last_error()
    assert L.pt_get_set_camera_times(C.byref(capi.PtSetCameraTimes())) != 0
    r = capi.Renderer(capi.Scene(paths["A"]), debug_flags=256)
    try:
        want_a = render_two_calls(r)
        t = r.set_camera_times()
        assert (t.tables_ms, t.rearm_ms, t.total_ms, t.path, t.fallback) == (0.0, 0.0, 0.0, 0, 0)  # no move yet
        before, bytes_before = r.read_tables(), r.stats().device_bytes
        assert L.pt_set_camera_ex(None, 2) != 0 and b"pt_set_camera_ex: null camera" in L.pt_last_error()  # the null camera comes before the flags
        for flags in (2, 3, 0x80000000):
            with pytest.raises(capi.PtError, match=r"pt_set_camera_ex: undefined flag bit\(s\) 0x%x" % (flags & ~1)):
                capi._check(L.pt_set_camera_ex(C.byref(cam_b), flags))
        wrong = capi.Scene(paths["B"]).camera
        wrong.resolution[0] = 97
        with pytest.raises(capi.PtError, match=r"undefined flag bit"):  # ... and before the resolution
            capi._check(L.pt_set_camera_ex(C.byref(wrong), 2))
        with pytest.raises(capi.PtError, match=r"pt_set_camera_ex: resolution 97x64 differs from the renderer's 96x64.*pt_init"):
            capi._check(L.pt_set_camera_ex(C.byref(wrong), 1))
        wrong = capi.Scene(paths["B"]).camera
        wrong.view[1] = float("inf")
        with pytest.raises(capi.PtError, match=r"pt_set_camera_ex: camera view\[1\] is not finite"):
            capi._check(L.pt_set_camera_ex(C.byref(wrong), 1))
        # nothing changed, nothing allocated, nothing cleared
        st = r.stats()
        assert r.read_tables() == before and st.device_bytes == bytes_before and st.samples == r.n * 8
        assert r.setup_times().set_camera_calls == 0 and np.array_equal(bits(r.readback()), bits(want_a))
        # flags == 0 is pt_set_camera: the same tables, the same image, no device copy of anything
        capi._check(L.pt_set_camera_ex(C.byref(cam_b), 0))
        assert times_of(r) == (0, 0)
        plain_tables, plain_img = r.read_tables(), render_two_calls(r)
        r.set_camera(capi.Scene(paths["A"]).camera)
        r.set_camera(cam_b)
        assert r.read_tables() == plain_tables and np.array_equal(bits(render_two_calls(r)), bits(plain_img))
        assert plain_tables != before and r.stats().device_bytes == bytes_before
        t = r.set_camera_times()
        assert t.total_ms == r.setup_times().set_camera_ms and t.tables_ms > 0 and t.rearm_ms > 0 and t.tables_ms + t.rearm_ms <= t.total_ms * 1.001
    finally:
        r.free()


def test_a_cell_longer_than_the_device_build_takes_falls_back(tmp_path, monkeypatch):
    """ptct::kDeviceMaxList = 4096 records in a cell of a forced grid (the host refuses such a grid unless it is forced): 4400 tiny
    primitives within one cell.  The host path runs, says why, and the tables are the host's."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes
    monkeypatch.setattr(grid_rays, "CROWD", dict(grid_rays.CROWD, n=4400))
    sc = capi.Scene(scenes.write_scene(grid_rays.scene_text("crowded", res=(96, 54)), str(tmp_path / "crowded4400.txt")))
    home, moved = sc.camera, sc.camera
    moved.position[2] += 1.5
    r = capi.Renderer(sc, debug_flags=256)
    try:
        assert r.grid_info()[1] > 4096
        r.set_camera(moved)
        host = r.read_tables()
        r.set_camera(home)
        r.set_camera(moved, device_tables=True)
        t = r.set_camera_times()
        assert (t.path, t.fallback) == (0, capi.PT_DEVICE_TABLES_LIST)
        assert r.read_tables() == host
        assert r.grid_info()[1] > 4096
    finally:
        r.free()


# ---- 7. the command-line front end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, "0,0"], ids=["single", "group"])
def test_orbit_with_device_tables_writes_the_same_frames(tmp_path, devices):
    """`pt_render --orbit N --device-tables`: the frames of the plain orbit, bit for bit, and the split of every move beside its line."""
    import os
    import re
    import subprocess
    from test_gpu_set_camera_cli import BIN, read_pfm
    path = scene_path(tmp_path, random_text, "A")
    frames, runs = 3, {}
    for name, extra in (("host", []), ("device", ["--device-tables"])):
        out = str(tmp_path / name)
        cmd = [BIN, path, "--orbit", str(frames), "--spp", "3", "--out", out, "--pfm"] + extra + (["--devices", devices] if devices else [])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        runs[name] = (p.stdout, [read_pfm(f"{out}.3samp.orbit{f:03d}.pfm")[0] for f in range(frames)])
    plain = r"^orbit: frame (\d+): camera \S+ \S+ \S+, set_camera \S+ ms, render \S+ ms"
    assert len(re.findall(plain + "$", runs["host"][0], re.M)) == frames  # without the flag the line is what it was
    assert len(re.findall(plain + "$", runs["device"][0], re.M)) == 1     # frame 0 has no move
    split = re.findall(plain + r", tables (\S+) ms, rearm (\S+) ms \((device|host) tables\)$", runs["device"][0], re.M)
    assert [m[0] for m in split] == ["1", "2"] and all(float(m[1]) > 0 and float(m[2]) > 0 and m[3] == "device" for m in split)
    for f in range(frames):
        assert np.array_equal(bits(runs["host"][1][f]), bits(runs["device"][1][f])), f
    assert not np.array_equal(bits(runs["device"][1][1]), bits(runs["device"][1][0]))
    p = subprocess.run([BIN, path, "--device-tables"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--device-tables goes with --orbit" in p.stderr
    assert not os.path.exists(str(tmp_path / "device") + ".3samp.png")
