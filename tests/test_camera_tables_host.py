"""Moving the camera of a live renderer, the host half (no GPU): the rebuild of the camera-dependent scene tables that
pt_set_camera runs (csrc/pt_tables.cpp camera_tables, through pt_camera_tables_host) against a fresh build of the tables for the
new camera, byte for byte; and the orbit state of the scene side (pt_scene_orbit: the reference's mouse rules, main.cpp:192-199,
followed by its camchanged block, main.cpp:112-126)."""
import ctypes as C
import math

import numpy as np
import pytest

from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes
from camera_scenes import cornell_text, random_text, scene_path, stress_text


def scene_at(tmp_path, text_fn, eye_name):
    return capi.Scene(scene_path(tmp_path, text_fn, eye_name))


def cam_bytes(cam):
    return bytes(memoryview(cam).cast("B"))


def test_default_eye_leaves_the_generated_text_unchanged():
    assert scenes.cornell_scene_text() == scenes.cornell_scene_text(eye=None, lookat=None)
    assert "EYE         0.0 5 10.5\nLOOKAT      0 5 0\n" in scenes.random_scene_text(3, 40)
    assert "EYE         0 5 30\n" in scenes.stress_scene_text(grid=(2, 2, 2), eye=(0, 5, 30))


@pytest.mark.parametrize("center_half", [0, 1])
@pytest.mark.parametrize("text_fn, flags", [(cornell_text, 0), (cornell_text, 256), (random_text, 0), (random_text, 256), (random_text, 2048),
                                            (stress_text, 0)])
def test_rebuilt_tables_equal_fresh_tables(tmp_path, text_fn, flags, center_half):
    """A -> each of B, C, D, E and back to A (the upper half of the mask), and each of them -> A."""
    home = scene_at(tmp_path, text_fn, "A")
    for name in "ABCDE":
        there = scene_at(tmp_path, text_fn, name)
        res, tight, differing = capi.camera_tables_host(home, there.camera, flags, center_half)
        assert differing == 0, (text_fn.__name__, flags, center_half, name, hex(differing))
        res, tight, differing = capi.camera_tables_host(there, home.camera, flags, center_half)
        assert differing == 0, (text_fn.__name__, flags, center_half, name, "-> A", hex(differing))


@pytest.mark.parametrize("flags", [0, 256])
def test_tightened_leaves_follow_the_camera(tmp_path, flags):
    home = scene_at(tmp_path, random_text, "A")
    counts = [capi.camera_tables_host(home, scene_at(tmp_path, random_text, name).camera, flags, 1)[1] for name in "ABCDE"]
    assert counts == [22, 21, 0, 0, 23]
    assert capi.camera_tables_host(home, home.camera, 2048, 1)[1] == 0  # the reference's boxes kept
    stress = scene_at(tmp_path, stress_text, "A")
    assert [capi.camera_tables_host(stress, scene_at(tmp_path, stress_text, name).camera, 0, 0)[1] for name in "AB"] == [149, 62]


def test_grid_keeps_the_resolution_of_init(tmp_path):
    home = scene_at(tmp_path, random_text, "A")
    res = {name: capi.camera_tables_host(home, scene_at(tmp_path, random_text, name).camera, 256, 0)[0] for name in "ABCDE"}
    assert res["A"] == res["B"] == res["E"] == (4, 4, 4)
    assert res["C"] == (4, 4, 4)  # the cost model alone says 3 x 3 x 3 there:
    far = scene_at(tmp_path, random_text, "C")
    assert capi.camera_tables_host(far, far.camera, 256, 0)[0] == (3, 3, 3)
    assert res["D"] == (0, 0, 0)  # no grid can be built; the BVH scan serves
    assert capi.camera_tables_host(home, home.camera, 0, 0)[0] == (0, 0, 0)  # 91 nodes: no grid candidate without the flag


def test_refuses_null_arguments(tmp_path):
    home = scene_at(tmp_path, cornell_text, "A")
    res, tight, differing = (C.c_int32 * 3)(), C.c_int32(), C.c_int32()
    assert capi.lib().pt_camera_tables_host(C.byref(home.desc), None, 0, 0, res, C.byref(tight), C.byref(differing)) != 0
    assert b"pt_camera_tables_host" in capi.lib().pt_last_error()


# ---- the scene side -------------------------------------------------------------------------------------------------------------
def test_orbit_by_nothing_is_the_identity_on_the_bits(tmp_path):
    for text_fn, name in ((cornell_text, "A"), (random_text, "B"), (cornell_text, "D")):
        s = scene_at(tmp_path, text_fn, name)
        before, state = cam_bytes(s.camera), s.orbit_state
        for _ in range(3):
            assert cam_bytes(s.orbit(0.0, 0.0, 0.0)) == before
        assert s.orbit_state == state and cam_bytes(s.desc.camera) == before


@pytest.mark.parametrize("steps", [4, 8])
def test_a_full_turn_returns_the_camera(tmp_path, steps):
    """Within 1e-5: a tolerance on libm's sinf / cosf and on steps float additions to phi, not a bit claim."""
    s = scene_at(tmp_path, cornell_text, "A")
    start = s.camera
    positions = []
    for _ in range(steps):
        positions.append(tuple(s.orbit(np.float32(2 * math.pi / steps), 0.0, 0.0).position))
    end = s.camera
    assert len(set(positions)) == steps  # it did move
    for field in ("position", "view", "up", "right", "lookAt", "fov", "pixelLength"):
        a, b = np.array(list(getattr(start, field)), np.float64), np.array(list(getattr(end, field)), np.float64)
        assert np.abs(a - b).max() <= 1e-5, (field, a, b)
    assert tuple(start.resolution) == tuple(end.resolution)


def test_orbit_moves_on_a_sphere_around_lookat(tmp_path):
    s = scene_at(tmp_path, cornell_text, "A")
    phi, theta, zoom = s.orbit_state
    cam = s.orbit(0.5, -0.25, 2.0)
    phi2, theta2, zoom2 = s.orbit_state
    f32 = np.float32
    assert (phi2, theta2, zoom2) == (float(f32(phi) + f32(0.5)), float(f32(theta) - f32(0.25)), float(f32(zoom) + f32(2.0)))
    d = np.array(list(cam.position), np.float64) - np.array(list(cam.lookAt), np.float64)
    assert abs(np.linalg.norm(d) - zoom2) < 1e-5 * zoom2
    assert np.allclose(np.array(list(cam.view)), -d / np.linalg.norm(d), atol=1e-6)


def test_theta_and_zoom_clamp_as_the_viewer_does(tmp_path):
    s = scene_at(tmp_path, cornell_text, "A")
    s.orbit(0.0, 10.0, 0.0)
    assert s.orbit_state[1] == float(np.float32(3.1415926535897932))  # fmin(theta, PI)
    s.orbit(0.0, -10.0, 0.0)
    assert s.orbit_state[1] == float(np.float32(0.001))               # fmax(0.001f, .)
    s.orbit(0.0, 0.0, -100.0)
    assert s.orbit_state[2] == float(np.float32(0.1))                 # fmax(0.1f, zoom)
    assert np.isfinite(np.array(list(s.camera.position))).all()
