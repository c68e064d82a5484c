"""The camera-dependent scene tables, the host half after their per-element arithmetic moved into csrc/pt_camera_tables.h (one
implementation for pt_tables.cpp and the kernels of pt_camera_tables.hip; no GPU): the rebuild still equals a fresh build byte for
byte, and pt_traversal_boxes / pt_center_half_box still give the bytes they gave before the move.  Those bytes are a fixture,
tests/golden/camera_tables_boxes.npz, recorded ONCE from the commit before the shared header existed (`python
tests/test_camera_tables_shared_host.py --record` with that commit's library): it pins "the refactor moved no bit" to something
other than the code under test.  Recording it again from a later commit would defeat it."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):  # (for --record; under pytest both are on the path already)
    if _p not in sys.path:
        sys.path.append(_p)
from camera_scenes import cornell_text, random_text, scene_path, stress_text  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_tables_boxes.npz")
CASES = [(random_text, "ABCDE", True), (stress_text, "AB", False)]  # (scene, cameras, with the centre / half extent forms)


def boxes_of(path, center_half):
    """What the two host entry points give for the scene file: the traversal boxes [n, 6], the tightened count, and the centre / half
    extent form of every box as a leaf and as an inner box (magnitude: the camera's largest coordinate, a float32)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(path)
    boxes, tight = scene.traversal_boxes()
    mag = np.float32(max(abs(v) for v in scene.desc.camera.position))
    fp = C.POINTER(C.c_float)
    if not center_half:
        return dict(boxes=boxes, tight=np.array([tight], np.int32))
    leaf, inner = np.zeros_like(boxes), np.zeros_like(boxes)
    for out, is_inner in ((leaf, 0), (inner, 1)):
        for i in range(boxes.shape[0]):
            lo, hi = np.ascontiguousarray(boxes[i, :3]), np.ascontiguousarray(boxes[i, 3:])
            c, h = np.zeros(3, np.float32), np.zeros(3, np.float32)
            capi.lib().pt_center_half_box(lo.ctypes.data_as(fp), hi.ctypes.data_as(fp), is_inner, C.c_float(mag), c.ctypes.data_as(fp),
                                          h.ctypes.data_as(fp))
            out[i, :3], out[i, 3:] = c, h
    return dict(boxes=boxes, tight=np.array([tight], np.int32), leaf=leaf, inner=inner)


def compute(tmp_path):
    out = {}
    for text_fn, names, center_half in CASES:
        for name in names:
            for key, value in boxes_of(scene_path(tmp_path, text_fn, name), center_half).items():
                out[f"{text_fn.__name__}_{name}_{key}"] = value
    return out


@pytest.fixture(scope="module")
def computed(tmp_path_factory):
    return compute(tmp_path_factory.mktemp("camera_tables_shared"))


def test_boxes_equal_the_bytes_recorded_before_the_shared_header(computed):
    want = np.load(GOLDEN)
    assert sorted(want.files) == sorted(computed)
    for key in want.files:
        a, b = np.ascontiguousarray(want[key]), np.ascontiguousarray(computed[key])
        assert a.dtype == b.dtype and a.shape == b.shape, key
        assert a.tobytes() == b.tobytes(), (key, np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(a.shape[0], -1).any(axis=1))[:8])


def test_the_fixture_covers_tightened_and_untouched_leaves(computed):
    """The recorded boxes exercise both outcomes of sphere_tight_box (near cameras tighten leaves, the far ones none) and both forms
    of center_half_box."""
    tight = {n: int(computed[f"random_text_{n}_tight"][0]) for n in "ABCDE"}
    assert tight["A"] > 0 and tight["E"] > 0 and tight["D"] == 0, tight
    assert not np.array_equal(computed["random_text_A_boxes"], computed["random_text_D_boxes"])
    assert not np.array_equal(computed["random_text_A_inner"], computed["random_text_A_leaf"])


@pytest.mark.parametrize("center_half", [0, 1])
@pytest.mark.parametrize("text_fn, flags", [(cornell_text, 0), (cornell_text, 256), (random_text, 0), (random_text, 256), (random_text, 2048),
                                            (stress_text, 0)])
def test_rebuilt_tables_still_equal_fresh_tables(tmp_path, text_fn, flags, center_half):
    """The scenes and cameras of test_camera_tables_host.py: A -> each camera and back, and each camera -> A."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    home = capi.Scene(scene_path(tmp_path, text_fn, "A"))
    for name in "ABCDE":
        there = capi.Scene(scene_path(tmp_path, text_fn, name))
        assert capi.camera_tables_host(home, there.camera, flags, center_half)[2] == 0, (text_fn.__name__, flags, center_half, name)
        assert capi.camera_tables_host(there, home.camera, flags, center_half)[2] == 0, (text_fn.__name__, flags, center_half, name, "-> A")


def test_tightened_counts_and_resolutions_are_unchanged(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    home = capi.Scene(scene_path(tmp_path, random_text, "A"))
    got = [capi.camera_tables_host(home, capi.Scene(scene_path(tmp_path, random_text, n)).camera, 256, 1)[:2] for n in "ABCDE"]
    assert [t for _, t in got] == [22, 21, 0, 0, 23]
    assert [r for r, _ in got] == [(4, 4, 4), (4, 4, 4), (4, 4, 4), (0, 0, 0), (4, 4, 4)]
    stress = capi.Scene(scene_path(tmp_path, stress_text, "A"))
    assert [capi.camera_tables_host(stress, capi.Scene(scene_path(tmp_path, stress_text, n)).camera, 0, 0)[1] for n in "AB"] == [149, 62]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_camera_tables_shared_host.py --record   (only with the library of the commit before csrc/pt_camera_tables.h)")
    from pathlib import Path
    with tempfile.TemporaryDirectory() as td:
        np.savez_compressed(GOLDEN, **compute(Path(td)))
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
