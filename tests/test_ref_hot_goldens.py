"""The hot path pinned to the reference's OWN code: oracle and product host code against the goldens that
oracle/ref_hot_harness.cpp (src/intersections.h, src/scene.cpp, src/utilities.cpp compiled in place) and
oracle/ref_rng_harness.cpp (rocThrust's minstd_rand / uniform_real_distribution) emitted.  CPU only; bit for bit."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest

import golden_io as gio
from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = os.path.join(HERE, "golden", "scenes")


@pytest.fixture(scope="module")
def isect():
    return gio.load("ref_isect.bin.gz")


@pytest.fixture(scope="module")
def rng():
    return gio.load("ref_rng.bin.gz")


def test_golden_volume(isect):
    """VERDICT r2 #1 asked for >= 20 k (geom, ray) vectors; count what the fixture holds and how many are hits."""
    total = hits = 0
    for s, (ng, nr) in enumerate(isect["sets"]):
        h = isect[f"hits_{s}"]
        assert h.shape == (ng * nr, 8) and isect[f"rays_{s}"].shape == (nr, 6) and isect[f"geoms_{s}"].shape == (ng, 50)
        total += len(h)
        hits += int((gio.f32(h[:, 0]) > 0).sum())
    assert total >= 20000 and hits >= 3000, (total, hits)  # a ray meets 1-2 of a scene's 7-9 primitives


def test_utilhash_matches_reference(isect, oracle):
    L = oracle.lib()
    got = np.array([L.orc_utilhash(int(a)) for a in isect["hash_in"][:, 0]], np.uint32)
    assert np.array_equal(got, isect["hash_out"][:, 0])
    kat = dict(zip(isect["hash_in"][:, 0].tolist(), isect["hash_out"][:, 0].tolist()))
    assert (kat[0], kat[1], kat[12345]) == (1800329511, 3028713910, 3058842707)  # SURVEY §4, now from the reference itself


def test_seed_expression_matches_reference_hash(isect, oracle):
    L = oracle.lib()
    got = np.array([L.orc_seed(int(i), int(p), int(d)) & 0xFFFFFFFF for i, p, d in isect["seed_in"].astype(np.int64)],
                   np.uint32)
    assert np.array_equal(got, isect["seed_out"][:, 0])


def test_rng_matches_rocthrust(rng, oracle):
    """thrust::default_random_engine(h) + uniform_real_distribution<float>(0, 1): five draws per seed, raw and float."""
    L = oracle.lib()
    raw = np.zeros(5, np.uint32)
    u = np.zeros(5, np.float32)
    seeds = rng["seed"][:, 0]
    assert len(seeds) >= 1500
    for k, s in enumerate(seeds):
        L.orc_rng_draws(C.c_int32(int(np.int32(s))), 5, raw.ctypes.data_as(C.POINTER(C.c_uint32)),
                        u.ctypes.data_as(C.POINTER(C.c_float)))
        assert np.array_equal(raw, rng["raw"][k]), (k, s)
        assert np.array_equal(u.view(np.uint32), rng["u01"][k]), (k, s)
    chk = rng["minstd_check"][0]
    assert chk[0] == 399268537 and chk[1] == 1 and chk[2] == 2147483646  # the C++ standard's check value; SURVEY §4
    assert L.orc_minstd_nth(1, 10000) == 399268537 and chk[3] == 48271
    ext = rng["extreme"]
    for sd, r, ub in ext:
        L.orc_rng_draws(C.c_int32(int(np.int32(sd))), 1, raw.ctypes.data_as(C.POINTER(C.c_uint32)),
                        u.ctypes.data_as(C.POINTER(C.c_float)))
        assert raw[0] == r and u.view(np.uint32)[0] == ub, (sd, r)
    uf = gio.f32(ext[:, 2])
    assert (uf == 1.0).any() and (uf == 0.0).any() and uf.max() <= 1.0  # u01 can round up to exactly 1 (SURVEY a-8)


def _install(oracle, geoms_tab):
    """Feed the reference loader's geom tables (type, materialid, three matrices) to the oracle unchanged."""
    from oracle import binding as ob
    ng = len(geoms_tab)
    arr = (ob.OrcGeom * ng)()
    for i, row in enumerate(geoms_tab):
        arr[i].type, arr[i].materialid = int(row[0]), int(row[1])
        f = gio.f32(row[2:])
        arr[i].transform[:] = f[0:16].tolist()
        arr[i].inverseTransform[:] = f[16:32].tolist()
        arr[i].invTranspose[:] = f[32:48].tolist()
    mats = (ob.OrcMaterial * 8)()
    cam = ob.OrcCamera()
    cam.res[0], cam.res[1] = 8, 8
    oracle.lib().orc_scene_set(arr, ng, mats, 8, C.byref(cam), 4)


@pytest.mark.parametrize("s", [0, 1])
def test_primitive_tests_match_reference(isect, oracle, s):
    """boxIntersectionTest / sphereIntersectionTest of intersections.h:48-144 on every (ray, geom) pair of the set:
    t, and for hits the point, the normal and `outside`, bit for bit."""
    ng, nr = (int(x) for x in isect["sets"][s])
    _install(oracle, isect[f"geoms_{s}"])
    rays = gio.f32(isect[f"rays_{s}"])
    want = isect[f"hits_{s}"].reshape(nr, ng, 8)
    L = oracle.lib()
    fp = C.POINTER(C.c_float)
    p = np.zeros(3, np.float32)
    n = np.zeros(3, np.float32)
    out = C.c_int(0)
    bad = []
    for r in range(nr):
        o = np.ascontiguousarray(rays[r, 0:3])
        d = np.ascontiguousarray(rays[r, 3:6])
        for g in range(ng):
            t = np.float32(L.orc_geom_test(g, o.ctypes.data_as(fp), d.ctypes.data_as(fp), p.ctypes.data_as(fp),
                                           n.ctypes.data_as(fp), C.byref(out)))
            w = want[r, g]
            ok = gio.same_bits_or_both_nan(np.array([t]).view(np.uint32), w[0:1]).all()
            if ok and gio.f32(w[0:1])[0] != -1.0:
                ok = (gio.same_bits_or_both_nan(p.view(np.uint32), w[1:4]).all()
                      and gio.same_bits_or_both_nan(n.view(np.uint32), w[4:7]).all() and int(out.value) == int(w[7]))
            if not ok:
                bad.append((r, g))
    assert not bad, bad[:10]


@pytest.mark.parametrize("s,name", [(0, "cornell.txt"), (1, "ref_twisted.txt")])
def test_closest_hit_from_golden_equals_oracle_traversal(isect, tmp_path, oracle, s, name):
    """computeIntersections as a whole: the closest hit assembled from the reference-compiled per-primitive results
    (+ the leaf-box filter, golden_io.expected_closest_hits) equals the oracle's BVH traversal on the same rays."""
    path = _scene_paths(tmp_path)[name]
    oracle.load_scene(path)
    rows, geom = gio.expected_closest_hits(isect, s, oracle.bvh())
    rays = gio.f32(isect[f"rays_{s}"])
    got = oracle.intersect(np.ascontiguousarray(rays[:, 0:3].T), np.ascontiguousarray(rays[:, 3:6].T))
    hit = geom >= 0
    assert hit.sum() > 800
    assert np.array_equal(got["t"] > 0, hit) and np.array_equal(got["geom"][hit], geom[hit])
    assert np.array_equal(got["t"][hit].view(np.uint32), rows[hit, 0])
    assert gio.same_bits_or_both_nan(got["pt"].T[hit].view(np.uint32), rows[hit, 1:4]).all()
    assert gio.same_bits_or_both_nan(got["nrm"].T[hit].view(np.uint32), rows[hit, 4:7]).all()
    assert np.array_equal(got["outside"][hit], rows[hit, 7].astype(np.int32))


def _scene_paths(tmp_path):
    """cornell.txt / sphere.txt are synthesised (the GPU box has no reference; scenes.py emits text that parses to the
    same tables — checked here against the golden of the reference's own files); the two fixtures are read in place."""
    return {
        "cornell.txt": scenes.write_scene(scenes.cornell_scene_text(), str(tmp_path / "cornell.txt")),
        "sphere.txt": scenes.write_scene(scenes.sphere_scene_text(), str(tmp_path / "sphere.txt")),
        "ref_twisted.txt": os.path.join(SCENES, "ref_twisted.txt"),
        "ref_quirks.txt": os.path.join(SCENES, "ref_quirks.txt"),
    }


def _u32(v):
    return np.array(v, np.uint32)


def test_loader_matches_reference_loader(tmp_path, oracle):
    """new Scene(path) of scene.cpp:7-188 — geoms, materials, camera, render state — against the oracle's loader (camera
    BEFORE main.cpp's fix-up, `right` = NaN included) and the product's (pt_scene_load applies the fix-up, so only the
    fields it leaves alone are compared for the camera)."""
    gold = json.load(open(os.path.join(HERE, "golden", "ref_scene.json")))
    paths = _scene_paths(tmp_path)
    assert [s["file"] for s in gold["scenes"]] == list(paths)
    for s in gold["scenes"]:
        path = paths[s["file"]]
        oracle.load_scene(path, fixup=False)
        sc = capi.Scene(path)
        for who, geoms, mats in (("oracle", oracle.geoms(), oracle.materials()), ("product", sc.geoms(), sc.materials())):
            assert len(geoms) == len(s["geoms"]) and len(mats) == len(s["materials"]), (who, s["file"])
            for g, w in zip(geoms, s["geoms"]):
                assert (g.type, g.materialid) == (w["type"], w["materialid"]), (who, s["file"])
                for k in ("transform", "inverseTransform", "invTranspose"):
                    got = np.frombuffer(bytes(getattr(g, k)), np.uint32)
                    assert gio.same_bits_or_both_nan(got, _u32(w[k])).all(), (who, s["file"], k)
            for m, w in zip(mats, s["materials"]):
                got = np.frombuffer(bytes(m), np.uint32)
                exp = np.concatenate([_u32(w[k]) for k in ("color", "specular_exponent", "specular_color", "hasReflective",
                                                           "hasRefractive", "indexOfRefraction", "emittance")])
                assert np.array_equal(got, exp), (who, s["file"])
        c, w = oracle.camera(), s["camera"]
        assert list(c.res) == w["resolution"]
        for k, field in (("position", c.position), ("lookAt", c.lookAt), ("view", c.view), ("up", c.up),
                         ("right", c.right), ("fov", c.fov), ("pixelLength", c.pixelLength)):
            got = np.frombuffer(bytes(field), np.uint32)
            assert gio.same_bits_or_both_nan(got, _u32(w[k])).all(), (s["file"], k)
        assert np.isnan(gio.f32(_u32(w["right"]))).all()  # scene.cpp:138 uses `view` before :142 assigns it
        pc = sc.desc.camera
        assert list(pc.resolution) == w["resolution"]
        for k, field in (("lookAt", pc.lookAt), ("fov", pc.fov), ("pixelLength", pc.pixelLength)):
            assert np.array_equal(np.frombuffer(bytes(field), np.uint32), _u32(w[k])), (s["file"], k)
        assert oracle.trace_depth() == sc.trace_depth == s["traceDepth"]
        assert oracle.lib().orc_iterations() == sc.iterations == s["iterations"]
        assert oracle.lib().orc_image_name().decode() == sc.image_name == s["imageName"]
        assert s["image_size"] == w["resolution"][0] * w["resolution"][1]


def test_isect_golden_geoms_are_the_loaders(isect, tmp_path, oracle):
    """The geom tables inside ref_isect.bin came out of the reference loader; our loaders produce the same tables, so
    the primitive-test parity above holds for scenes loaded by the product as well."""
    paths = _scene_paths(tmp_path)
    for s, name in enumerate(["cornell.txt", "ref_twisted.txt"]):
        sc = capi.Scene(paths[name])
        tab = isect[f"geoms_{s}"]
        assert sc.desc.num_geoms == len(tab)
        for g, row in zip(sc.geoms(), tab):
            got = np.frombuffer(bytes(g), np.uint32)
            assert gio.same_bits_or_both_nan(got, row).all()


def test_synthesised_scene_text_equals_reference_files():
    """What scenes.py emits parses like the reference's own files: token streams equal line by line (the reference's
    streams pinned by their SHA-256 in tests/golden/ref_scene_tokens.json, made by `make -C oracle goldens`)."""
    gold = json.load(open(os.path.join(HERE, "golden", "ref_scene_tokens.json")))["sha256_of_scene_tokens"]
    for name, text in (("cornell.txt", scenes.cornell_scene_text()), ("sphere.txt", scenes.sphere_scene_text())):
        assert gio.scene_tokens_digest(text) == gold[name], name


@pytest.mark.skipif(not (os.path.isdir("/root/reference/src") and shutil.which("make")), reason="reference not mounted")
def test_goldens_regenerate_byte_for_byte(tmp_path):
    """`make -C oracle goldens` output equals the committed fixtures (only where the reference is mounted)."""
    import subprocess
    orc = os.path.join(os.path.dirname(HERE), "oracle")
    subprocess.check_call(["make", "-C", orc, "ref"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    if not os.path.exists(os.path.join(orc, "_ref", "ref_hot")):
        pytest.skip("no <cuda_runtime.h> in this image")
    g = os.path.join(HERE, "golden")
    run = lambda *a: subprocess.check_call(list(a), stdout=subprocess.DEVNULL)
    run(os.path.join(orc, "_ref", "ref_hot"), "scene", str(tmp_path / "s.json"), "/root/reference/scenes/cornell.txt",
        "/root/reference/scenes/sphere.txt", os.path.join(SCENES, "ref_twisted.txt"), os.path.join(SCENES, "ref_quirks.txt"))
    assert open(tmp_path / "s.json", "rb").read() == open(os.path.join(g, "ref_scene.json"), "rb").read()
    run(os.path.join(orc, "_ref", "ref_hot"), "isect", str(tmp_path / "i.bin"), "/root/reference/scenes/cornell.txt",
        os.path.join(SCENES, "ref_twisted.txt"))
    import gzip
    assert open(tmp_path / "i.bin", "rb").read() == gzip.open(os.path.join(g, "ref_isect.bin.gz")).read()
    run(os.path.join(orc, "_ref", "ref_rng"), str(tmp_path / "i.bin"), str(tmp_path / "r.bin"))
    assert open(tmp_path / "r.bin", "rb").read() == gzip.open(os.path.join(g, "ref_rng.bin.gz")).read()
