"""Host logic of the product without a GPU: the C ABI loads and exports every declared symbol, the
C++ scene loader / BVH builder / transform builder agree bit-for-bit with the oracle and with the
reference-built goldens, the PNG writer honours saveImage()'s semantics, and render entry points
fail loudly (no CPU fallback)."""
import json
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_every_declared_symbol_is_exported():
    hdr = open(os.path.join(ROOT, "include", "pt_amd.h")).read()
    names = set(re.findall(r"\b(pt_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) >= 20
    L = capi.lib()
    for n in sorted(names):
        assert hasattr(L, n), f"{n} declared in include/pt_amd.h but not exported by libpt_amd.so"


def test_struct_sizes_match_reference_layouts():
    import ctypes as C
    # sceneStructs.h: Material 44 B, Camera 84 B; pathtrace.cu: BVHNodeGPU 36 B
    assert C.sizeof(capi.PtMaterial) == 44 and C.sizeof(capi.PtCamera) == 84 and C.sizeof(capi.PtBVHNode) == 36
    assert C.sizeof(capi.PtGeom) == 8 + 3 * 64


def test_options_struct_size_matches_header():
    import ctypes as C
    # include/pt_amd.h PtOptions: 20 int32 fields (pt_api.cpp asserts the same size)
    assert C.sizeof(capi.PtOptions) == 80


@pytest.mark.parametrize("name,res", [("cornell", None), ("cornell", (1920, 1080)), ("sphere", (256, 256)), ("stress", None)])
def test_scene_tables_match_oracle(scene_dir, oracle, name, res):
    sc = capi.Scene(scene_dir[name], res=res)
    oracle.load_scene(scene_dir[name], res=res)
    assert bytes(sc.desc.camera) == bytes(oracle.camera())
    assert sc.desc.num_geoms == len(oracle.geoms()) and sc.desc.num_materials == len(oracle.materials())
    assert all(bytes(a) == bytes(b) for a, b in zip(sc.geoms(), oracle.geoms()))
    assert all(bytes(a) == bytes(b) for a, b in zip(sc.materials(), oracle.materials()))
    assert all(bytes(a) == bytes(b) for a, b in zip(sc.bvh(), oracle.bvh()))
    assert sc.trace_depth == oracle.trace_depth() == 8
    assert len(sc.bvh()) == 2 * sc.desc.num_geoms - 1


def test_scene_metadata_and_errors(scene_dir, tmp_path):
    sc = capi.Scene(scene_dir["cornell"])
    assert sc.resolution == (800, 800) and sc.iterations == 1000 and sc.image_name == "cornell"
    with pytest.raises(capi.PtError):
        capi.Scene(str(tmp_path / "nope.txt"))


def test_transforms_match_reference_build():
    xf = json.load(open(os.path.join(HERE, "golden", "ref_xforms.json")))
    for x in xf["xforms"]:
        trs = np.array(x["trs"], np.uint32).view(np.float32)
        m, i, it = capi.build_transform(trs)
        assert np.array_equal(m.view(np.uint32), np.array(x["transform"], np.uint32))
        assert np.array_equal(i.view(np.uint32), np.array(x["inverse"], np.uint32))
        assert np.array_equal(it.view(np.uint32), np.array(x["invTranspose"], np.uint32))


def test_large_scene_bvh_matches_oracle(tmp_path, oracle):
    """~1000 primitives on a regular grid: many equal centroids, so the tree depends on std::sort's
    tie order (the reference uses std::sort; product and oracle both call it)."""
    p = scenes.write_scene(scenes.stress_scene_text((10, 10, 10)), str(tmp_path / "s.txt"))
    sc = capi.Scene(p)
    oracle.load_scene(p)
    a, b = sc.bvh(), oracle.bvh()
    assert len(a) == len(b) == 2 * 1006 - 1
    assert all(bytes(x) == bytes(y) for x, y in zip(a, b))


def _decode_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert zlib.crc32(typ + body) & 0xFFFFFFFF == crc
        if typ == b"IHDR":
            w, h, bd, ct = struct.unpack(">IIBB", body[:10])
            assert (bd, ct) == (8, 2)
        elif typ == b"IDAT":
            idat += body
        pos += 12 + n
    raw = zlib.decompress(idat)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3)


def test_png_writer_matches_saveimage_semantics(tmp_path):
    """main.cpp:86-107 + image.cpp:22-39: divide by samples, mirror x, clamp to [0,1], *255, truncate; no gamma."""
    w, h, spp = 37, 11, 4.0
    rng = np.random.default_rng(0)
    img = rng.uniform(-0.5, 6.0, (h * w, 3)).astype(np.float32)
    img[5] = [np.nan, 4.0, 2.0]
    p = str(tmp_path / "o.png")
    capi.save_png(p, img, w, h, spp)
    got = _decode_png(p)
    avg = img.reshape(h, w, 3) / np.float32(spp)
    with np.errstate(invalid="ignore"):
        exp = (np.minimum(np.maximum(np.nan_to_num(avg, nan=0.0), 0), 1) * np.float32(255)).astype(np.uint8)[:, ::-1]
    assert np.array_equal(got, exp)
    capi.save_pfm(str(tmp_path / "o.pfm"), img, w, h, spp)
    raw = open(tmp_path / "o.pfm", "rb").read()
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    assert raw.startswith(head)
    body = np.frombuffer(raw[len(head):], np.float32).reshape(h, w, 3)[::-1]
    assert np.array_equal(body.view(np.uint32), avg.view(np.uint32))


def test_png_writer_matches_reference_compiled_writer(tmp_path):
    """tests/golden/ref_image.json holds what the REFERENCE's image writer (src/image.cpp + src/stb.cpp compiled in place,
    oracle/ref_image_harness.cpp, filled like saveImage() main.cpp:91-97) put into its PNG for an image with negatives,
    zeros, exactly 1, values around byte boundaries, > 1, infinities and a NaN: pt_save_png must write the same pixels."""
    g = json.load(open(os.path.join(HERE, "golden", "ref_image.json")))
    w, h = g["width"], g["height"]
    img = np.array(g["sum_bits"], np.uint32).view(np.float32).reshape(h * w, 3)
    p = str(tmp_path / "g.png")
    capi.save_png(p, img, w, h, float(g["samples"]))
    assert np.array_equal(_decode_png(p), np.array(g["png_rgb8"], np.uint8).reshape(h, w, 3))


def test_output_basename_is_the_reference_file_name():
    """main.cpp:99-102: <FILE>.<UTC start time %Y-%m-%d_%H-%M-%Sz>.<samples as streamed float>samp; one start time per process."""
    a = capi.output_basename("cornell", 5000)
    assert re.fullmatch(r"cornell\.\d{4}-\d\d-\d\d_\d\d-\d\d-\d\dz\.5000samp", a), a
    b = capi.output_basename("x", 1000000)
    assert b.endswith(".1e+06samp") and b.split(".")[1] == a.split(".")[1]


def test_no_cpu_fallback_without_gpu(scene_dir):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    sc = capi.Scene(scene_dir["cornell"], res=(16, 16))
    with pytest.raises(capi.PtError):
        capi.Renderer(sc)
    with pytest.raises(capi.PtError):
        capi._check(capi.lib().pt_render(1, 1))
    capi.pt_free()  # legal before init


def test_product_never_touches_oracle():
    """The product tree must not reference oracle/ (only the oracle includes the shared math header)."""
    pkg = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip", ".hpp")) or f == "Makefile":
                txt = open(os.path.join(d, f), errors="replace").read()
                assert "liboracle" not in txt and "oracle.binding" not in txt and "from oracle" not in txt, os.path.join(d, f)


def test_kernel_build_has_no_compile_time_switches():
    """Product constants are constexpr, not overridable macros: the only identifiers the preprocessor tests are the
    arithmetic mode, the diagnostic PT_WALK_STATS build and the compiler's own; the Makefile defines PT_ARITH alone.
    A new switch needs a deliberate edit of this list."""
    csrc = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "csrc")
    tested = set()
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".inc", ".h")):
            for line in open(os.path.join(csrc, f), errors="replace"):
                m = re.match(r"\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)", line)
                if m:
                    cond = re.sub(r"//.*|/\*.*?\*/", "", m.group(1))
                    tested |= set(re.findall(r"\b[A-Za-z_]\w*", cond)) - {"defined"}
    assert "PT_ARITH" in tested
    assert tested <= {"PT_ARITH", "PT_WALK_STATS", "__HIPCC__"}, sorted(tested)
    make = open(os.path.join(csrc, "Makefile")).read()
    assert set(re.findall(r"-D\s*(\w+)", make)) == {"PT_ARITH"}


def test_scene_table_builder_needs_no_hip():
    """csrc/pt_tables.cpp, everything the renderer uploads for a scene, is plain C++: the system compiler, without any
    ROCm include path, accepts it, so no HIP header can creep into the builder."""
    src = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "csrc", "pt_tables.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


REF_TOKENS = os.path.join(HERE, "golden", "ref_scene_tokens.json")  # SHA-256 of the reference's scenes/*.txt token streams


def _with_comments(text: str) -> str:
    """The reference's scene files carry `// ...` comment lines before each block; the loader must skip them."""
    out = []
    for line in text.split("\n"):
        if line.startswith(("MATERIAL", "CAMERA", "OBJECT")):
            out.append("// " + line.lower() + " block")
        out.append(line)
    return "\n".join(out)


@pytest.mark.parametrize("name", ["cornell", "sphere"])
def test_comment_lines_are_skipped(oracle, name, scene_dir, tmp_path):
    text = open(scene_dir[name]).read()
    path = scenes.write_scene(_with_comments(text), str(tmp_path / (name + "_c.txt")))
    a, b = capi.Scene(path), capi.Scene(scene_dir[name])
    oracle.load_scene(path)
    assert bytes(a.desc.camera) == bytes(b.desc.camera) == bytes(oracle.camera())
    assert all(bytes(x) == bytes(y) for x, y in zip(a.geoms(), b.geoms()))
    assert all(bytes(x) == bytes(y) for x, y in zip(a.materials(), b.materials()))
    assert all(bytes(x) == bytes(y) for x, y in zip(a.bvh(), oracle.bvh()))


@pytest.mark.parametrize("name", ["cornell", "sphere"])
def test_reference_scene_files_parse_like_the_synthesised_ones(oracle, name, scene_dir, tmp_path):
    """scenes.py must describe exactly the reference's scenes/*.txt: the reference's file is the synthesised text token
    for token (REF_TOKENS) in the reference's layout, `// ...` lines before each block; that layout must give the same
    camera, geometry, materials, iteration count, depth and output name through the product loader and the oracle loader."""
    import golden_io as gio
    text = open(scene_dir[name]).read()
    assert gio.scene_tokens_digest(text) == json.load(open(REF_TOKENS))["sha256_of_scene_tokens"][name + ".txt"]
    path = scenes.write_scene(_with_comments(text), str(tmp_path / (name + ".txt")))
    sc, syn = capi.Scene(path), capi.Scene(scene_dir[name])
    oracle.load_scene(path)
    assert bytes(sc.desc.camera) == bytes(syn.desc.camera) == bytes(oracle.camera())
    assert sc.desc.num_geoms == syn.desc.num_geoms and sc.desc.num_materials == syn.desc.num_materials
    assert all(bytes(a) == bytes(b) for a, b in zip(sc.geoms(), syn.geoms()))
    assert all(bytes(a) == bytes(b) for a, b in zip(sc.materials(), syn.materials()))
    assert all(bytes(a) == bytes(b) for a, b in zip(sc.bvh(), oracle.bvh()))
    assert sc.iterations == syn.iterations and sc.trace_depth == syn.trace_depth and sc.image_name == syn.image_name


def test_save_hdr_bytes_equal_the_reference_writer(tmp_path):
    """tests/golden/ref_hdr.json: the files the REFERENCE's image::saveHDR (src/image.cpp:41-45 + stb, compiled in place by
    oracle/ref_image_harness.cpp, filled like saveImage()) wrote for a 300-pixel-wide image (run-length path: runs longer
    than 127, literal stretches longer than 128, tiny / huge / zero pixels) and a 5-pixel-wide one (flat RGBE).
    pt_save_hdr writes the same bytes."""
    g = json.load(open(os.path.join(HERE, "golden", "ref_hdr.json")))
    assert len(g["cases"]) == 2
    for case in g["cases"]:
        w, h = case["width"], case["height"]
        s = np.array(case["sum_bits"], np.uint32).view(np.float32).reshape(h * w, 3)
        path = str(tmp_path / f"o{w}.hdr")
        capi.save_hdr(path, s, w, h, g["samples"])
        got = open(path, "rb").read()
        want = bytes.fromhex(case["hdr_file_hex"])
        assert got[:80] == want[:80]
        assert got == want, f"{w}x{h}: first difference at byte {next(i for i, (a, b) in enumerate(zip(got, want)) if a != b) if len(got) == len(want) else (len(got), len(want))}"
