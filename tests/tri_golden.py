"""tests/golden/ref_tri.bin.gz for the tests that use it: the golden of oracle/ref_tri_harness.cpp (the reference's vendored
glm::intersectRayTriangle and its getPointOnRay, compiled in place) and the scene of its 24 triangles."""
import numpy as np

import golden_io as gio
from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes

FAMILIES = ("face", "edge", "vertex", "hair", "back", "grazing", "on plane", "axis", "far")
NTRI, NRAYS = 24, 1024
SMALL = (14, 15, 16, 17)  # the triangles whose a = dot(e1, cross(d, e2)) straddles FLT_EPSILON

_gold = None


def gold():
    """The sections as uint32 arrays, plus: rays o, d [3, n] float32, family / target / feature [n]."""
    global _gold
    if _gold is None:
        g = gio.load("ref_tri.bin.gz")
        assert g["tris"].shape == (NTRI, 9) and g["rays_0"].shape == (NRAYS, 6) and g["sets"].tolist() == [[NTRI, NRAYS]]
        assert g["bary"].shape == (NTRI * NRAYS, 4) and g["hits_0"].shape == (NTRI * NRAYS, 8)
        rays = gio.f32(g["rays_0"])
        info = g["rayinfo"].astype(np.int64)
        g.update(o=np.ascontiguousarray(rays[:, 0:3].T), d=np.ascontiguousarray(rays[:, 3:6].T), family=info[:, 0], target=info[:, 1],
                 feature=info[:, 2])
        for v in g.values():
            v.setflags(write=False)
        _gold = g
    return _gold


def family(name):
    return gold()["family"] == FAMILIES.index(name)


def write_scene(path, **kw):
    return scenes.write_scene(scenes.triangle_table_scene_text(gio.f32(gold()["tris"]).tolist(), **kw), str(path))


def load_scene(path):
    """capi.Scene of a file written by write_scene, after the precondition of every test on it: the loader hands back the
    golden's vertices bit for bit (the golden holds no -0.0, which alone may come back changed)."""
    sc = capi.Scene(str(path))
    tris = gold()["tris"]
    assert not (tris == 0x80000000).any()
    geoms = sc.geoms()
    assert sc.desc.num_geoms >= NTRI
    for k in range(NTRI):
        assert geoms[k].type == 2 and geoms[k].materialid == 1 + k % 4
        got = np.frombuffer(bytes(geoms[k].transform), np.uint32)[0:9]
        assert np.array_equal(got, tris[k]), (k, gio.f32(got), gio.f32(tris[k]))
    return sc
