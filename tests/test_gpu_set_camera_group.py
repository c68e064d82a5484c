"""pt_group_set_camera: every context of a group moves to the new camera, or none does."""
import numpy as np
import pytest

from camera_scenes import scene_path
from cosc_4397_pathtracing_raytracing_project_amd import scenes

pytestmark = pytest.mark.gpu
RES = (96, 60)


def cornell_text(eye=None):
    return scenes.cornell_scene_text(res=RES, eye=eye)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def single(path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(path))
    try:
        r.render(1, 8)
        return r.readback()
    finally:
        r.free()


def test_group_moves_every_context_or_none(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    paths = {n: scene_path(tmp_path, cornell_text, n) for n in "AB"}
    want = {n: single(paths[n]) for n in "AB"}
    assert not np.array_equal(bits(want["A"]), bits(want["B"]))
    g = capi.Group(capi.Scene(paths["A"]), [0, 0, 0], transport="copy")
    try:
        g.render(1, 8)
        assert np.array_equal(bits(g.gather()), bits(want["A"]))
        # a camera one context would refuse changes no context
        bad = capi.Scene(paths["B"], res=(96, 61)).camera
        with pytest.raises(capi.PtError, match=r"pt_group_set_camera: resolution 96x61 differs from the renderer's 96x60.*pt_init"):
            g.set_camera(bad)
        bad = capi.Scene(paths["B"]).camera
        bad.up[1] = float("inf")
        with pytest.raises(capi.PtError, match=r"pt_group_set_camera: camera up\[1\] is not finite"):
            g.set_camera(bad)
        assert np.array_equal(bits(g.gather()), bits(want["A"]))  # nothing was cleared
        for i in range(3):
            t = capi.PtSetupTimes()
            capi._check(capi.lib().pt_ctx_get_setup_times(g.context(i), capi.C.byref(t)))
            assert t.set_camera_calls == 0
        g.render(9, 8)  # and the view is still A: iterations 9 .. 16 on top of 1 .. 8, as a single renderer adds them
        r = capi.Renderer(capi.Scene(paths["A"]))
        try:
            r.render(1, 8)
            r.render(9, 8)
            sixteen = r.readback()
        finally:
            r.free()
        assert np.array_equal(bits(g.gather()), bits(sixteen))
        # the move itself
        g.set_camera(capi.Scene(paths["B"]).camera)
        assert not g.gather().any()
        g.render(1, 8)
        assert np.array_equal(bits(g.gather()), bits(want["B"]))
        g.set_camera(capi.Scene(paths["A"]).camera)
        g.render(1, 8)
        assert np.array_equal(bits(g.gather()), bits(want["A"]))
    finally:
        g.free()
