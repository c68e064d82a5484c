"""The mesh extension's triangle test pinned to the reference's OWN vendored code: the oracle's triangleIntersectionTest against
tests/golden/ref_tri.bin.gz, which oracle/ref_tri_harness.cpp made with glm::intersectRayTriangle (external/include/glm/gtx/
intersect.inl:37-74) and getPointOnRay (src/intersections.h:27-29) compiled in place.  CPU only; bit for bit.

Pinned by the golden: GLM's hit / miss decision and its distance baryPosition.z (and .x, .y, section `bary`).  The extension's own
convention, which the harness restates with the reference's functions: the point pulled back by getPointOnRay, the normal
normalize(cross(e1, e2)), the returned distance length(origin - point)."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import golden_io as gio
import tri_golden as tg

HERE = os.path.dirname(os.path.abspath(__file__))


def _facing(g):
    """[rays, triangles]: the triangle's front (the side cross(e1, e2) points to) faces the ray, in float64."""
    tris = gio.f32(g["tris"]).astype(np.float64).reshape(tg.NTRI, 3, 3)
    n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    return -(g["d"].T.astype(np.float64) @ n.T) > 0


def _at_the_aim(g):
    """[rays, triangles]: the triangle has the edge / the vertex that the ray aims at (the target itself and the triangles
    that share the feature's vertices bit for bit)."""
    tris = g["tris"].reshape(tg.NTRI, 3, 3)
    out = np.zeros((tg.NRAYS, tg.NTRI), bool)
    has = lambda k, v: (tris[k] == v).all(axis=1).any()
    for r in range(tg.NRAYS):
        k, f = int(g["target"][r]), int(g["feature"][r])
        want = [tris[k, f]] if g["family"][r] == tg.FAMILIES.index("vertex") else [tris[k, f], tris[k, (f + 1) % 3]]
        out[r] = [all(has(j, v) for v in want) for j in range(tg.NTRI)]
    return out


def test_golden_inputs_are_decided_both_ways():
    """Counts of the golden itself: they guard the inputs, not the code."""
    g = tg.gold()
    hit = g["bary"].reshape(tg.NRAYS, tg.NTRI, 4)[:, :, 0] == 1
    t = gio.f32(g["hits_0"][:, 0]).reshape(tg.NRAYS, tg.NTRI)
    assert np.array_equal(hit, t != -1.0) and np.array_equal(hit, g["hits_0"][:, 7].reshape(tg.NRAYS, tg.NTRI) == 1)
    assert [int(tg.family(f).sum()) for f in tg.FAMILIES] == [160, 192, 96, 192, 96, 96, 96, 48, 48]
    rows = np.arange(tg.NRAYS)
    # rays aimed at an edge, at a vertex or a hair beside an edge, against the triangles that have that edge / vertex and face the ray
    close = (tg.family("edge") | tg.family("vertex") | tg.family("hair"))[:, None] & _at_the_aim(g) & _facing(g)
    print(f"edge / vertex / hair pairs facing the ray: {int(close.sum())}, hits {hit[close].mean():.3f}")
    assert close.sum() >= 480 and hit[close].mean() >= 0.2 and (~hit[close]).mean() >= 0.2
    back = tg.family("back")
    assert not hit[back, g["target"][back]].any()  # front faces only
    for k in tg.SMALL:  # a straddles FLT_EPSILON: among the rays that look at the triangle's front
        mine = (g["target"] == k) & ~back & _facing(g)[:, k]
        assert hit[mine, k].any() and (~hit[mine, k]).any(), k
    z = gio.f32(g["bary"][:, 3]).reshape(tg.NRAYS, tg.NTRI)
    assert (hit & (z < 1e-4)).any()  # t - 1e-4 of either sign
    assert hit[tg.family("face"), g["target"][tg.family("face")]].mean() >= 0.5 and hit.sum() >= 1000
    assert np.isfinite(gio.f32(g["hits_0"][:, 0:7])).all()


@pytest.mark.parametrize("mode", ["LIBM", "PORTABLE"])
def test_oracle_triangle_test_matches_glm(oracle, tmp_path, mode):
    """orc_geom_test on every one of the 24,576 (ray, triangle) pairs: hit / miss, distance bits, point and normal."""
    g = tg.gold()
    path = tg.write_scene(tmp_path / "tri.txt")
    tg.load_scene(path)
    oracle.set_math_mode(getattr(oracle, mode))
    oracle.load_scene(path)
    og = oracle.geoms()
    assert len(og) == tg.NTRI
    for k in range(tg.NTRI):
        assert np.array_equal(np.frombuffer(bytes(og[k].transform), np.uint32)[0:9], g["tris"][k])
    want = g["hits_0"].reshape(tg.NRAYS, tg.NTRI, 8)
    o, d = np.ascontiguousarray(g["o"].T), np.ascontiguousarray(g["d"].T)
    bad = []
    for r in range(tg.NRAYS):
        for k in range(tg.NTRI):
            t, p, n, outside = oracle.geom_test(k, o[r], d[r])
            w = want[r, k]
            ok = bool(gio.same_bits_or_both_nan(np.array([t]).view(np.uint32), w[0:1]).all())
            if ok and gio.f32(w[0:1])[0] != -1.0:
                ok = bool(gio.same_bits_or_both_nan(p.view(np.uint32), w[1:4]).all()
                          and gio.same_bits_or_both_nan(n.view(np.uint32), w[4:7]).all() and outside == int(w[7]))
            if not ok:
                bad.append((r, tg.FAMILIES[g["family"][r]], k))
    assert not bad, (len(bad), bad[:10])


def test_closest_hit_from_golden_equals_oracle_traversal(oracle, tmp_path):
    """The whole search on the scene of the 24 triangles: the closest hit assembled from GLM's per-triangle results behind the
    padded leaf boxes (golden_io.expected_closest_hits) equals the oracle's traversal."""
    g = tg.gold()
    path = tg.write_scene(tmp_path / "tri.txt")
    tg.load_scene(path)
    oracle.load_scene(path)
    rows, geom = gio.expected_closest_hits(g, 0, oracle.bvh())
    got = oracle.intersect(g["o"], g["d"])
    hit = geom >= 0
    assert hit.sum() >= 500 and (~hit).sum() >= 100
    assert np.array_equal(got["t"] > 0, hit) and np.array_equal(got["geom"][hit], geom[hit])
    assert np.array_equal(got["t"][hit].view(np.uint32), rows[hit, 0])
    assert gio.same_bits_or_both_nan(got["pt"].T[hit].view(np.uint32), rows[hit, 1:4]).all()
    assert gio.same_bits_or_both_nan(got["nrm"].T[hit].view(np.uint32), rows[hit, 4:7]).all()


@pytest.mark.skipif(not (os.path.isdir("/root/reference/src") and shutil.which("make")), reason="reference not mounted")
def test_golden_regenerates_byte_for_byte(tmp_path):
    orc = os.path.join(os.path.dirname(HERE), "oracle")
    subprocess.check_call(["make", "-C", orc, "ref"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    if not os.path.exists(os.path.join(orc, "_ref", "ref_tri")):
        pytest.skip("no <cuda_runtime.h> in this image")
    subprocess.check_call([os.path.join(orc, "_ref", "ref_tri"), str(tmp_path / "t.bin")], stdout=subprocess.DEVNULL)
    assert open(tmp_path / "t.bin", "rb").read() == gzip.open(os.path.join(HERE, "golden", "ref_tri.bin.gz")).read()
