"""The uniform-grid walk (LABNOTES.md section 9.1) on scenes chosen to stress the cell walk itself: flat layouts (one cell
along an axis), huge extents, axis-parallel rays that run exactly along cell boundaries, a camera inside the grid, objects
much larger and much smaller than a cell, no walls at all.  Grid forced (debug_flags 256) against the oracle bit for bit,
and against the BVH scan (512).  The everyday scenes are in tests/test_gpu_render.py / test_mesh_extension.py."""
import os

import numpy as np
import pytest

from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def scene_text(objects, res, eye, lookat, depth=8):
    out = [scenes._material(i, **m) for i, m in enumerate(scenes._CORNELL_MATERIALS)]
    out.append(scenes._camera(res, 45, 8, depth, "grid", eye, lookat, (0, 1, 0)))
    for i, (kind, mat, t, r, s) in enumerate(objects):
        out.append(scenes._object(i, kind, mat, t, r, s))
    return "".join(out)


def layouts():
    rnd = np.random.RandomState(5)
    flat = [("cube", 0, (0, 6, 0), (0, 0, 0), (3, ".1", 3))]  # a light above a sheet of primitives in the plane y = 0
    for ix in range(-6, 7):
        for iz in range(-6, 7):
            flat.append(("sphere" if (ix + iz) & 1 else "cube", 1 + (ix * 7 + iz) % 4, (ix * 0.8, 0, iz * 0.8), (0, 0, 0), (".5", ".5", ".5")))
    far = [("cube", 0, (0, 4000, 0), (0, 0, 0), (6000, 10, 6000))]  # extent ~1e4: coordinates where float spacing is ~1e-3
    for k in range(120):
        far.append(("sphere" if k & 1 else "cube", 1 + k % 4, tuple(np.round(rnd.uniform(-3000, 3000, 3), 1)), tuple(rnd.randint(0, 90, 3)),
                    tuple(np.round(rnd.uniform(100, 600, 3), 1))))
    # axis-aligned cubes on an exact lattice, camera looking straight down the z axis through the middle: primary and
    # mirror-bounce rays with zero direction components, running along cell boundaries
    lattice = [("cube", 0, (0, 9, 0), (0, 0, 0), (20, ".2", 20)), ("cube", 4, (0, 0, -8), (0, 0, 0), (16, 16, ".2"))]
    for ix in range(-3, 4):
        for iy in range(-3, 4):
            for iz in range(-3, 4):
                if (ix, iy) != (0, 0):
                    lattice.append(("cube", 1 + (ix + iy + iz) % 3, (ix * 2, iy * 2, iz * 2), (0, 0, 0), (1, 1, 1)))
    mixed = [("cube", 0, (0, 12, 0), (0, 0, 0), (8, ".2", 8)), ("sphere", 4, (0, 0, 0), (0, 0, 0), (14, 14, 14)),  # one primitive as large as the scene
             ("cube", 1, (0, -9, 0), (0, 0, 0), (30, ".5", 30))]
    for k in range(200):
        mixed.append(("sphere" if k % 3 else "cube", 1 + k % 4, tuple(np.round(rnd.uniform(-9, 9, 3), 2)), tuple(rnd.randint(0, 180, 3)),
                      tuple(np.round(rnd.uniform(0.02, 0.3, 3), 3))))  # and many far smaller than a cell
    # a small scene (extent ~ 12) ten thousand units from the origin, camera beside it: |coordinate| / extent ~ 1e3, where
    # 1e-4 * extent would be one ulp of a coordinate (the pad has to follow the coordinate magnitude)
    off = np.array([10000.0, 9000.0, -10000.0])
    offset = [("cube", 0, tuple(off + (0, 6, 0)), (0, 0, 0), (4, ".25", 4)), ("cube", 1, tuple(off + (0, -6, 0)), (0, 0, 0), (12, ".25", 12))]
    for k in range(150):
        offset.append(("sphere" if k & 1 else "cube", 1 + k % 4, tuple(np.round(off + rnd.uniform(-5, 5, 3), 2)), tuple(rnd.randint(0, 90, 3)),
                       tuple(np.round(rnd.uniform(0.2, 0.9, 3), 2))))
    return {
        "offset": (offset, tuple(off + (0.5, 1, 16)), tuple(off)),
        "flat": (flat, (0, 4, 9), (0, 0, 0)),
        "far": (far, (0, 500, 9000), (0, 0, 0)),
        "lattice_axis_rays": (lattice, (0, 0, 30), (0, 0, 0)),
        "inside": (lattice, (1, 1, 1), (0.3, 8, -5)),  # camera inside the grid, between the cubes
        "mixed_sizes": (mixed, (0, 2, 25), (0, 0, 0)),
    }


@pytest.mark.parametrize("name", ["flat", "far", "lattice_axis_rays", "inside", "mixed_sizes", "offset"])
def test_forced_grid_on_unusual_layouts(oracle, tmp_path, name):
    objects, eye, lookat = layouts()[name]
    res, spp = (128, 96), 4
    path = scenes.write_scene(scene_text(objects, res, eye, lookat), str(tmp_path / f"{name}.txt"))
    sc = capi.Scene(path, res=res)
    info = sc.grid(forced=True)[0]
    imgs = {}
    for flags in (256, 512):
        r = capi.Renderer(sc, debug_flags=flags)
        try:
            r.render(1, spp)
            imgs[flags] = r.readback()
            assert (r.stats().grid_cells > 0) == (flags == 256)
        finally:
            r.free()
    assert np.isfinite(imgs[256]).all()
    oracle.set_math_mode(oracle.PORTABLE)
    oracle.load_scene(path, res=res)
    ref = oracle.render(1, spp, depth=8, variant=oracle.RETIRE, nthreads=min(16, os.cpu_count() or 1))
    diff = (bits(imgs[256]) != bits(ref)).any(axis=1)
    assert not diff.any(), f"{name} (grid {list(info.res)}): {diff.sum()} pixels differ from the oracle, first {np.flatnonzero(diff)[:8]}"
    assert np.array_equal(bits(imgs[256]), bits(imgs[512]))
    assert (imgs[256].sum(axis=1) > 0).mean() > 0.05, "the camera sees the scene"


@pytest.mark.parametrize("layout", ["lattice", "mixed_sizes", "offset", "room"])
@pytest.mark.parametrize("arith", ["fma", "fast"])
def test_grid_and_scan_give_the_same_image_in_every_mode(tmp_path, arith, layout):
    """The structure only changes which leaves are LOOKED AT, never which pass their box test: the fma / fast images are
    identical with either structure too (same kernels' arithmetic on the same candidates).  The grid tests leaf boxes only, so
    it is the flat side of the fused kernels; the scan tests inner boxes on the way — in the fast build with the slack of
    center_half_box, which has to cover primitives far smaller than the scene (mixed_sizes, room: grazing_rays.py) and
    coordinates far larger than it (offset)."""
    if layout == "lattice":
        res, spp = (160, 90), 6
        text = scenes.stress_scene_text((10, 10, 8), res=res)
    elif layout == "room":
        import grazing_rays
        res, spp = (128, 96), 4
        text = grazing_rays.scene_text("room", res=res)
    else:
        res, spp = (128, 96), 4
        objects, eye, lookat = layouts()[layout]
        text = scene_text(objects, res, eye, lookat)
    path = scenes.write_scene(text, str(tmp_path / "s.txt"))
    sc = capi.Scene(path, res=res)
    imgs = []
    for flags in (256, 512):
        r = capi.Renderer(sc, debug_flags=flags, arith=arith)
        try:
            r.render(1, spp)
            imgs.append(r.readback())
            assert (r.stats().grid_cells > 0) == (flags == 256)
        finally:
            r.free()
    assert np.isfinite(imgs[0]).all() and (imgs[0].sum(axis=1) > 0).mean() > 0.05, "the camera sees the scene"
    assert np.array_equal(bits(imgs[0]), bits(imgs[1]))


def test_striped_tiles_on_the_grid_compose(scene_dir):
    """The multi-GPU partition (row-interleaved tiles, global pixel indices in the RNG) with the grid walk in both fused
    kernels: every rank's rows, scattered back, give the single-context image bit for bit."""
    from cosc_4397_pathtracing_raytracing_project_amd import parallel
    res, spp = (96, 50), 4
    w, h = res
    sc = capi.Scene(scene_dir["stress_big"], res=res)

    def render(**kw):
        r = capi.Renderer(sc, debug_flags=256, **kw)
        try:
            r.render(1, spp)
            assert r.stats().grid_cells > 0
            return r.readback()
        finally:
            r.free()

    full = render()
    for world in (2, 5):
        out = np.zeros((h, w, 3), np.float32)
        for rank in range(world):
            out[rank::world] = render(**parallel.striped_tile_for_rank(w, h, rank, world)).reshape(-1, w, 3)
        assert np.array_equal(bits(out.reshape(-1, 3)), bits(full))


@pytest.mark.parametrize("clustered", [False, True])
def test_init_time_choice_among_structures_never_changes_the_image(oracle, tmp_path, clustered):
    """pt_init times the BVH scan, the cost model's grid and two finer grids on a large scene and keeps the fastest
    (choose_traversal); sphere leaves are tested against their tightened boxes (PtStats.tight_leaves).  Whatever it picks:
    the exact-mode image equals the oracle's — which walks the reference's tree over the reference's boxes — bit for bit, and
    equals the images with the grid forced / forbidden and with the reference's boxes kept (debug_flags 2048)."""
    res, spp = (240, 160), 3
    path = scenes.write_scene(scenes.random_scene_text(31 + clustered, 1400, res=res, depth=8, clustered=clustered), str(tmp_path / "r.txt"))
    sc = capi.Scene(path, res=res)
    imgs, tight = {}, {}
    for flags in (0, 256, 512, 2048, 256 | 2048):
        r = capi.Renderer(sc, debug_flags=flags)
        try:
            r.render(1, spp)
            imgs[flags] = r.readback()
            st = r.stats()
            tight[flags] = st.tight_leaves
            if flags & 256:
                assert st.grid_cells > 0
            if flags & 512:
                assert st.grid_cells == 0
        finally:
            r.free()
    assert tight[0] > 300 and tight[256] == tight[0] and tight[2048] == 0 and tight[256 | 2048] == 0
    oracle.set_math_mode(oracle.PORTABLE)
    oracle.load_scene(path, res=res)
    ref = oracle.render(1, spp, depth=8, variant=oracle.RETIRE, nthreads=min(16, os.cpu_count() or 1))
    for flags, img in imgs.items():
        assert np.array_equal(bits(img), bits(ref)), f"debug_flags {flags}"


@pytest.mark.parametrize("layout", ["lattice", "random", "clustered"])
@pytest.mark.parametrize("arith", ["fma", "fast"])
def test_tightened_sphere_leaves_do_not_change_fma_and_fast_images(tmp_path, arith, layout):
    """The tightened boxes are sized for the float slop of the sphere test in the reference's arithmetic (x 4); the fma / fast
    tests round differently but no worse: same image with the reference's boxes (debug_flags 2048), grid and scan — on the
    lattice scene and on random / clustered scenes (rotated, non-uniformly scaled spheres; grazing hits at many angles)."""
    res, spp = (320, 200), 4
    text = {"lattice": lambda: scenes.stress_scene_text((12, 12, 10), res=res),
            "random": lambda: scenes.random_scene_text(31, 1200, res=res),
            "clustered": lambda: scenes.random_scene_text(32, 1500, res=res, clustered=True)}[layout]()
    path = scenes.write_scene(text, str(tmp_path / "s.txt"))
    sc = capi.Scene(path, res=res)
    imgs = []
    for flags in (256, 256 | 2048, 512, 512 | 2048):
        r = capi.Renderer(sc, debug_flags=flags, arith=arith)
        try:
            r.render(1, spp)
            imgs.append(r.readback())
            assert (r.stats().tight_leaves > 0) == (not flags & 2048)
        finally:
            r.free()
    for im in imgs[1:]:
        assert np.array_equal(bits(imgs[0]), bits(im))
