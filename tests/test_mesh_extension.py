"""Triangle `mesh` objects — an EXTENSION: the scene format names the type (INSTRUCTION.md:246) and the reference includes
<glm/gtx/intersect.hpp> (intersections.h:4), but neither its loader nor its kernels implement it.  The intersection decision and
distance are pinned to that header's compiled glm::intersectRayTriangle elsewhere (test_ref_tri_golden.py, test_gpu_mesh_pin.py); the
loader, the padded boxes and the rendering have nothing in the reference to compare with.  Tested here:
  * scenes without meshes are untouched (the rest of the suite);
  * loader: product == oracle byte for byte (triangle primitives, BVH with padded triangle boxes), OBJECT ids keep counting
    objects (a cube after two meshes is still accepted), the reference's scenes parse as before;
  * intersection = glm::intersectRayTriangle semantics (front faces only), checked on hand-computable rays;
  * GPU == oracle bit for bit in exact mode (LDS-table and global-table kernels, fused and unfused), fma / fast within the
    stated tolerance."""
import numpy as np
import pytest

from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture()
def mesh_scene(tmp_path):
    return scenes.write_scene(scenes.mesh_scene_text(), str(tmp_path / "mesh.txt"))


def test_loader_matches_oracle_and_counts_objects(oracle, mesh_scene):
    sc = capi.Scene(mesh_scene)
    oracle.load_scene(mesh_scene)
    geoms = sc.geoms()
    assert sc.desc.num_geoms == len(oracle.geoms()) == 7 + 8 + 8 + 2 + 1
    assert [g.type for g in geoms[:7]] == [1, 1, 1, 1, 1, 1, 0] and all(g.type == 2 for g in geoms[7:25]) and geoms[25].type == 1
    assert all(bytes(a) == bytes(b) for a, b in zip(geoms, oracle.geoms()))
    assert all(bytes(a) == bytes(b) for a, b in zip(sc.bvh(), oracle.bvh()))
    assert len(sc.bvh()) == 2 * 26 - 1
    for g in geoms[7:25]:  # vertices in transform[0..8], everything else zero
        assert not any(g.transform[9:]) and not any(g.inverseTransform) and not any(g.invTranspose)
    # the axis-aligned quad (z = -3 plane): its two triangles get boxes with thickness
    quad = [n for n in sc.bvh() if n.left < 0 and n.geomIndex in (23, 24)]
    assert len(quad) == 2 and all(n.bmax[2] > n.bmin[2] for n in quad)


def test_mesh_block_without_tri_lines_loads_like_the_reference_loader(oracle, tmp_path):
    """A reference-format file can say `mesh` (INSTRUCTION.md:246) but cannot contain TRI lines — those are this build's
    own syntax.  Such a block must load as the reference's loader leaves it (scene.cpp:47-55: no type assigned, ONE geom
    pushed): one geom, the initial type, the following objects' ids and indices unshifted."""
    text = scenes.cornell_scene_text(res=(32, 32))
    text += "OBJECT 7\nmesh\nmaterial 2\nTRANS 1 2 3\nROTAT 0 45 0\nSCALE 2 2 2\n\n"
    text += "OBJECT 8\ncube\nmaterial 3\nTRANS -1 1 0\nROTAT 0 0 0\nSCALE 1 1 1\n\n"
    path = scenes.write_scene(text, str(tmp_path / "m.txt"))
    sc = capi.Scene(path)
    oracle.load_scene(path)
    geoms = sc.geoms()
    assert sc.desc.num_geoms == len(oracle.geoms()) == 9
    assert geoms[7].type == 0 and geoms[7].materialid == 2 and geoms[8].type == 1 and geoms[8].materialid == 3
    assert all(bytes(a) == bytes(b) for a, b in zip(geoms, oracle.geoms()))
    m, i, it = capi.build_transform([1, 2, 3, 0, 45, 0, 2, 2, 2])
    assert np.array_equal(np.frombuffer(bytes(geoms[7].transform), np.float32), m)


def test_triangle_test_is_glm_intersect_ray_triangle(oracle, mesh_scene):
    """The quad faces +z (towards the camera): rays from the front hit it at z = -3 with normal (0, 0, 1); rays from behind
    pass through (front faces only, like glm::intersectRayTriangle); rays beside it miss."""
    oracle.load_scene(mesh_scene)
    o = np.array([[0.0, 8.0, 5.0], [0.0, 8.0, -4.9], [1.9, 8.9, 5.0], [2.1, 8.0, 5.0]], np.float32).T.copy()
    d = np.array([[0, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, -1]], np.float32).T.copy()
    h = oracle.intersect(o, d)
    quad_mat = 3
    assert h["mat"][0] == quad_mat and abs(h["t"][0] - (8.0 - 1e-4)) < 1e-5 and np.allclose(h["nrm"][:, 0], [0, 0, 1])
    assert abs(h["pt"][2, 0] - (-3.0 + 1e-4)) < 1e-5
    assert h["mat"][1] != quad_mat or h["t"][1] < 0 or abs(h["pt"][2, 1] + 3.0) > 1e-2  # from behind: not the quad
    assert h["mat"][2] == quad_mat                                                       # near its corner, still inside
    assert not (h["mat"][3] == quad_mat and abs(h["pt"][2, 3] + 3.0) < 1e-2)              # beside it


@pytest.mark.gpu
@pytest.mark.parametrize("grid,res,spp,kw", [
    (0, (200, 120), 7, {}),                              # 26 leaves: LDS-table kernels
    (0, (200, 120), 7, dict(unfused_primary=True)),
    (0, (200, 120), 7, dict(unfused_bounces=True, iters_per_batch=3)),
    (0, (97, 61), 5, dict(legacy_traversal=True)),
    (4, (160, 96), 4, {}),                               # 64 more octahedra = 538 leaves: global tables, subtree scans
    (4, (160, 96), 4, dict(unfused_bounces=True)),
    (4, (160, 96), 4, dict(debug_flags=256)),            # forced uniform-grid walk
])
def test_gpu_mesh_bit_exact_vs_oracle(oracle, tmp_path, grid, res, spp, kw):
    path = scenes.write_scene(scenes.mesh_scene_text(res=res, grid=grid), str(tmp_path / "m.txt"))
    r = capi.Renderer(capi.Scene(path, res=res), **kw)
    try:
        r.render(1, spp)
        img = r.readback()
    finally:
        r.free()
    oracle.set_math_mode(oracle.PORTABLE)
    oracle.load_scene(path, res=res)
    ref = oracle.render(1, spp, depth=8, variant=oracle.RETIRE, nthreads=16)
    assert np.isfinite(img).all()
    diff = (bits(img) != bits(ref)).any(axis=1)
    assert not diff.any(), f"{diff.sum()} pixels differ, first {np.flatnonzero(diff)[:8]}"


@pytest.mark.gpu
def test_gpu_mesh_stage_intersect(oracle, tmp_path):
    res = (320, 180)
    path = scenes.write_scene(scenes.mesh_scene_text(res=res, grid=3), str(tmp_path / "m.txt"))
    r = capi.Renderer(capi.Scene(path, res=res))
    try:
        oracle.load_scene(path, res=res)
        o, d = oracle.generate(0, res[0] * res[1])
        g, h = capi.Renderer.stage_intersect(o, d), oracle.intersect(o, d)
        for k in ("t", "nrm", "mat", "pt"):
            assert np.array_equal(bits(g[k]), bits(h[k])), k
        assert (h["mat"] >= 0).any()
    finally:
        r.free()


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["fma", "fast"])
def test_gpu_mesh_modes_within_tolerance(oracle, tmp_path, arith):
    res, spp = (200, 120), 8
    path = scenes.write_scene(scenes.mesh_scene_text(res=res), str(tmp_path / "m.txt"))
    r = capi.Renderer(capi.Scene(path, res=res), arith=arith)
    try:
        r.render(1, spp)
        img = r.readback()
    finally:
        r.free()
    oracle.set_math_mode(oracle.LIBM)
    oracle.load_scene(path, res=res)
    ref = oracle.render(1, spp, depth=8, variant=oracle.LITERAL, nthreads=16)
    oracle.set_math_mode(oracle.PORTABLE)
    alt = oracle.render(1, spp, depth=8, variant=oracle.LITERAL, nthreads=16)
    a, b = img / np.float32(spp), ref / np.float32(spp)
    floor = float((np.abs(alt / np.float32(spp) - b).max(axis=1) > 1e-5).mean())
    off = float((np.abs(a - b).max(axis=1) > 1e-5).mean())
    mse = np.mean((a.astype(np.float64) - b) ** 2)
    print(f"{arith} mesh scene: {100 * off:.3f} % off (floor {100 * floor:.3f} %), PSNR {10 * np.log10(1 / mse):.1f} dB")
    assert np.isfinite(a).all() and off <= 0.002 + 3 * floor and 10 * np.log10(1 / mse) >= 45


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [0, 4])  # LDS tables; global tables with subtree scans
@pytest.mark.parametrize("arith", ["fma", "fast"])
def test_gpu_mesh_fused_bounces_equal_the_unfused_stages(tmp_path, arith, grid):
    """What pt_stage_intersect sees is what k_paths renders: within fma and fast the mesh scene rendered by the fused bounce kernel
    equals the unfused intersect / shade stages bit for bit (test_gpu_arith.py asserts this for cornell, which has no triangle)."""
    res, spp = (200, 120) if grid == 0 else (160, 96), 6
    path = scenes.write_scene(scenes.mesh_scene_text(res=res, grid=grid), str(tmp_path / "m.txt"))
    imgs = []
    for kw in ({}, dict(unfused_bounces=True), dict(unfused_bounces=True, iters_per_batch=3)):
        r = capi.Renderer(capi.Scene(path, res=res), arith=arith, **kw)
        try:
            r.render(1, spp)
            imgs.append(r.readback())
        finally:
            r.free()
    assert np.isfinite(imgs[0]).all() and (imgs[0] > 0).any()
    for img, what in zip(imgs[1:], ("unfused_bounces", "unfused_bounces, batches of 3")):
        diff = (bits(imgs[0]) != bits(img)).any(axis=1)
        assert not diff.any(), f"{arith}, {what}: {diff.sum()} pixels differ, first {np.flatnonzero(diff)[:8]}"
