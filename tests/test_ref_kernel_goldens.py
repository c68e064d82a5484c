"""The __global__ bodies of src/pathtrace.cu — generateRayFromCamera :270-286, computeIntersections :288-333, shadeAndExtendRays
:336-437, finalGather :439-444 — and main.cpp's camera fix-up (:57-71, :110-128), pinned to the reference's OWN text:
oracle/ref_kernels_harness.cpp includes those line ranges, cut out of the files at build time, and `make -C oracle goldens`
writes the two fixtures read here (numbers only).  CPU tests: the oracle in LIBM mode, and the product's host-side camera code,
against them bit for bit; and the oracle in PORTABLE mode (what the GPU's exact build is bit-identical to) inside the
project's stated image tolerance of the reference's images."""
import gzip
import os
import shutil

import numpy as np
import pytest

import golden_io as gio
import ref_kernel_golden as rk
from cosc_4397_pathtracing_raytracing_project_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return rk.scene_paths(tmp_path_factory.mktemp("ref_kernel_scenes"))


def same(a, b) -> bool:
    return bool(gio.same_bits_or_both_nan(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)).all())


def first_diff(a, b):
    bad = ~gio.same_bits_or_both_nan(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    return np.argwhere(bad)[:8].tolist()


# ---- volume ---------------------------------------------------------------------------------------------------------------------
def test_golden_volume():
    k, im = rk.kernels(), rk.images()
    assert [len(k[s]) for s in ("cam_loaded", "cam_state0", "cam_fixed")] == [4, 4, 4]
    assert [k[f"orbit_{s}"].shape for s in range(4)] == [(31, 27)] * 4
    frames = [tuple(int(x) for x in r) for r in k["gen_frames"]]
    assert frames == [(0, 61, 37, 8), (0, 32, 32, 8), (0, 48, 32, 8), (1, 24, 16, 8), (1, 17, 23, 8), (2, 24, 16, 6), (2, 17, 23, 6),
                      (3, 24, 16, 5), (3, 17, 23, 5)]
    assert [len(k[f"gen_{i}"]) for i in range(len(frames))] == [w * h for _, w, h, _ in frames]
    assert [tuple(int(x) for x in r) for r in k["isect_sets"]] == [(0, 1536), (2, 1536)]
    assert k["isect_0"].shape == k["isect_1"].shape == (1536, 10)
    assert len(k["shade_in"]) == len(k["shade_out"]) == len(k["shade_branch"]) == 2674
    assert [c[1:] for c in rk.image_cases()] == [
        (0, 96, 64, 8, 1, 8), (0, 61, 37, 8, 1, 16), (0, 48, 32, 1, 1, 4), (0, 48, 32, 2, 1, 4), (0, 48, 32, 5, 1, 4), (0, 48, 32, 20, 1, 4),
        (1, 48, 32, 4, 1, 8), (2, 48, 32, 8, 1, 8), (3, 48, 32, 8, 1, 8), (0, 48, 32, 8, 4194300, 8), (0, 48, 32, 8, 2147483600, 4)]
    assert len(rk.IMAGE_IDS) == len(rk.image_cases())
    for c in rk.image_cases():
        assert im[f"sum_{c[0]}"].shape == (c[2] * c[3], 3)
    for name in ("ref_kernels.bin.gz", "ref_kernel_images.bin.gz"):  # no larger than the largest fixture there was before them
        assert os.path.getsize(os.path.join(gio.GOLDEN, name)) <= os.path.getsize(os.path.join(gio.GOLDEN, "ref_bvh_c5.bin.gz"))


def test_shade_vectors_reach_every_branch():
    """Every return of shadeAndExtendRays and every side of every condition, at least 50 vectors each; the committed counts are
    the masks' counts."""
    k, v = rk.kernels(), rk.shade_vectors()
    counts = k["shade_counts"][:, 0]
    assert len(counts) == len(rk.BRANCHES)
    for b, name in enumerate(rk.BRANCHES):
        assert counts[b] == rk.has(v["mask"], name).sum(), name
        assert counts[b] >= 50, (name, int(counts[b]))
    assert set(v["iter"]) >= {1, 4194303, 4194304, 2147483647}
    assert v["idx"].max() == 1920 * 1080 - 1 and v["idx"].min() == 0
    assert set(v["depth"]) >= {0, 3, 4, 63}
    # what the labels claim shows in the kernel's outputs
    killed = rk.has(v["mask"], "kill_d4") | rk.has(v["mask"], "kill_d63")
    assert (v["out_remaining"][killed] == 0).all() and same(v["out_color"][killed], v["color"][killed])
    last = rk.has(v["mask"], "last_bounce_scatters")
    assert (v["out_remaining"][last] == 0).all() and not same(v["out_d"][last], v["d"][last])
    dead = rk.has(v["mask"], "hit_dead")
    assert same(v["out_color"][dead], v["color"][dead]) and same(v["out_o"][dead], v["o"][dead]) and same(v["out_d"][dead], v["d"][dead])


# ---- camera ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", range(4), ids=rk.SCENE_NAMES)
def test_camera_fixup_matches_reference(paths, oracle, s):
    """main.cpp:57-71 and the camchanged block :110-128: the oracle's loader camera without the fix-up, and with it; the product's
    pt_scene_load camera and its orbit state."""
    k = rk.kernels()
    oracle.load_scene(paths[s], fixup=False)
    assert same(rk.camera_words(oracle.camera()), k["cam_loaded"][s]), first_diff(rk.camera_words(oracle.camera()), k["cam_loaded"][s])
    oracle.load_scene(paths[s], fixup=True)
    assert same(rk.camera_words(oracle.camera()), k["cam_fixed"][s]), first_diff(rk.camera_words(oracle.camera()), k["cam_fixed"][s])
    sc = capi.Scene(paths[s])
    assert same(rk.camera_words(sc.camera), k["cam_fixed"][s]), first_diff(rk.camera_words(sc.camera), k["cam_fixed"][s])
    assert same(rk.camera_words(sc.desc.camera), k["cam_fixed"][s])
    assert same(np.array(sc.orbit_state, np.float32), k["cam_state0"][s, 0:3])


@pytest.mark.parametrize("s", range(4), ids=rk.SCENE_NAMES)
def test_orbit_reaches_the_reference_cameras(paths, s):
    """pt_scene_orbit from the loaded scene: the drags reach the golden's states bit for bit (the float rule is the project's own),
    and the camera after each is what the reference's camchanged block makes of that state."""
    rows = rk.kernels()[f"orbit_{s}"]
    sc = capi.Scene(paths[s])
    theta, zoom = gio.f32(rows[:, 4]), gio.f32(rows[:, 5])
    assert (theta == np.float32(0.001)).any() and (theta == np.float32(np.pi)).any() and (zoom == np.float32(0.1)).any()
    for i, row in enumerate(rows):
        dphi, dtheta, dzoom = (float(x) for x in gio.f32(row[0:3]))
        cam = sc.orbit(dphi, dtheta, dzoom)
        assert same(np.array(sc.orbit_state, np.float32), row[3:6]), (i, sc.orbit_state)
        assert same(rk.camera_words(cam), row[6:27]), (i, first_diff(rk.camera_words(cam), row[6:27]))


# ---- generate, intersect, shade --------------------------------------------------------------------------------------------------
def test_generate_matches_reference_kernel(paths, oracle):
    k = rk.kernels()
    for i, (s, w, h, depth) in enumerate(tuple(int(x) for x in r) for r in k["gen_frames"]):
        g = k[f"gen_{i}"]
        oracle.load_scene(paths[s], res=(w, h))
        assert oracle.trace_depth() == depth
        o, d = oracle.generate(0, w * h)
        assert same(o.T, g[:, 0:3]) and same(d.T, g[:, 3:6]), (i, first_diff(d.T, g[:, 3:6]))
        assert (gio.f32(g[:, 6:9]) == 1.0).all() and np.array_equal(g[:, 9], np.arange(w * h)) and (g[:, 10] == depth).all()


@pytest.mark.parametrize("s", [0, 1])
def test_intersect_matches_reference_kernel(paths, oracle, s):
    """The whole of computeIntersections — stack order, dispatch, `t > 0 && t < t_min`, what a miss leaves — on ref_hot's rays."""
    k = rk.kernels()
    scene, n = (int(x) for x in k["isect_sets"][s])
    rays = gio.f32(gio.load("ref_isect.bin.gz")[f"rays_{s}"])
    assert len(rays) == n
    want = k[f"isect_{s}"]
    oracle.load_scene(paths[scene])
    got = oracle.intersect(rk.soa(rays[:, 0:3]), rk.soa(rays[:, 3:6]))
    hit = gio.f32(want[:, 0]) >= 0
    assert 800 < hit.sum() < n
    assert same(got["t"], want[:, 0]), first_diff(got["t"], want[:, 0])
    assert same(got["nrm"].T, want[:, 1:4]) and same(got["pt"].T, want[:, 5:8])
    assert np.array_equal(got["mat"], want[:, 4].astype(np.int32)) and np.array_equal(got["outside"], want[:, 8].astype(np.int32))
    assert np.array_equal(got["geom"][hit], want[hit, 9].astype(np.int32)) and (got["geom"][~hit] == -1).all()
    assert (want[~hit, 1:] == 0).all()  # a miss writes t alone; the rest is the memset's


def oracle_shade(oracle, v):
    """oracle.shade on all vectors (grouped by depth): out arrays in the vectors' order, and the colour after the replayed depths."""
    n = len(v["t"])
    out = dict(o=np.zeros((n, 3), np.float32), d=np.zeros((n, 3), np.float32), color=np.zeros((n, 3), np.float32),
               remaining=np.zeros(n, np.int32), replayed=np.zeros((n, 3), np.float32))
    for depth in sorted(set(v["depth"])):
        sel = np.flatnonzero(v["depth"] == depth)
        it, px, hit = np.ascontiguousarray(v["iter"][sel]), np.ascontiguousarray(v["idx"][sel]), rk.hit_of(v, sel)
        o, d, c, rem = oracle.shade(int(depth), it, px, hit, rk.soa(v["o"][sel]), rk.soa(v["d"][sel]), rk.soa(v["color"][sel]), v["remaining"][sel])
        out["o"][sel], out["d"][sel], out["color"][sel], out["remaining"][sel] = o.T, d.T, c.T, rem
        c2 = c.copy()
        for extra in range(1, int(v["remaining"][sel].max())):  # a missed path meets its miss again at every later depth
            more = (hit["t"] < 0) & (v["remaining"][sel] > extra)
            if more.any():
                sub = dict(t=hit["t"][more], nrm=np.ascontiguousarray(hit["nrm"][:, more]), mat=hit["mat"][more], pt=np.ascontiguousarray(hit["pt"][:, more]))
                c2[:, more] = oracle.shade(int(depth) + extra, it[more], px[more], sub, np.ascontiguousarray(o[:, more]), np.ascontiguousarray(d[:, more]),
                                           np.ascontiguousarray(c2[:, more]), np.ascontiguousarray(rem[more]))[2]
        out["replayed"][sel] = c2.T
    return out


def test_shade_matches_reference_kernel(oracle):
    """One shadeAndExtendRays call per vector: branch order, draw order, the rough mirror's two draws for one angle, the roulette
    from depth 4, the sky factor — the oracle in LIBM mode gives the kernel's segment bit for bit."""
    v = rk.shade_vectors()
    oracle.load_scene(rk.SHADE_SCENE)
    got = oracle_shade(oracle, v)
    assert np.array_equal(got["remaining"], v["out_remaining"]), np.flatnonzero(got["remaining"] != v["out_remaining"])[:8]
    for name in ("o", "d", "color"):
        assert same(got[name], v["out_" + name]), (name, first_diff(got[name], v["out_" + name]))
    assert same(got["replayed"], v["out_replayed"]), first_diff(got["replayed"], v["out_replayed"])


# ---- images ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rk.image_cases(), ids=rk.IMAGE_IDS)
def test_images_match_reference_loop(paths, oracle, case):
    """The SUM image of the harness's restated launch loop over the reference's kernels: the oracle in LIBM mode, both loop
    variants, one thread and eight, bit for bit — iterations past 2^22 (where iteration and depth bits of the seed overlap) and
    next to 2^31 included."""
    k, s, w, h, depth, first, count = case
    want = rk.images()[f"sum_{k}"]
    oracle.load_scene(paths[s], res=(w, h))
    for variant in (oracle.LITERAL, oracle.RETIRE):
        for nthreads in (1, 8):
            got = oracle.render(first, count, depth=depth, variant=variant, nthreads=nthreads)
            assert same(got, want), (variant, nthreads, first_diff(got, want))


@pytest.mark.parametrize("case", rk.image_cases(), ids=rk.IMAGE_IDS)
def test_portable_oracle_within_stated_tolerance_of_reference_images(paths, oracle, case):
    """The reference alone stays inside the cap the GPU tests use: PORTABLE differs from the reference's compiled code through
    sin / cos / acos only."""
    k, s, w, h, depth, first, count = case
    oracle.load_scene(paths[s], res=(w, h))
    oracle.set_math_mode(oracle.PORTABLE)
    got = oracle.render(first, count, depth=depth, variant=oracle.RETIRE, nthreads=8)
    rk.check_stated_tolerance(got, gio.f32(rk.images()[f"sum_{k}"]), count, f"portable-oracle {rk.IMAGE_IDS[k]}")


# ---- regeneration ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not (os.path.isdir("/root/reference/src") and shutil.which("make")), reason="reference not mounted")
def test_ref_kernel_goldens_regenerate_byte_for_byte(tmp_path):
    import subprocess
    orc = os.path.join(os.path.dirname(HERE), "oracle")
    subprocess.check_call(["make", "-C", orc, "ref"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    exe = os.path.join(orc, "_ref", "ref_kernels")
    if not os.path.exists(exe):
        pytest.skip("no <cuda_runtime.h> in this image")
    g = os.path.join(HERE, "golden")
    with open(tmp_path / "i.bin", "wb") as f:
        f.write(gzip.open(os.path.join(g, "ref_isect.bin.gz")).read())
    ref = "/root/reference/scenes/"
    tail = [str(tmp_path / "i.bin"), rk.SHADE_SCENE, ref + "cornell.txt", ref + "sphere.txt", os.path.join(g, "scenes", "ref_twisted.txt"),
            os.path.join(g, "scenes", "ref_quirks.txt")]
    for modes, name in (("camera,generate,intersect,shade", "ref_kernels.bin.gz"), ("images", "ref_kernel_images.bin.gz")):
        out = str(tmp_path / "o.bin")
        subprocess.check_call([exe, modes, out] + tail, stdout=subprocess.DEVNULL)
        assert open(out, "rb").read() == gzip.open(os.path.join(g, name)).read(), name
        raw = subprocess.check_output(["gzip", "-9nc", out])
        assert raw == open(os.path.join(g, name), "rb").read(), name
