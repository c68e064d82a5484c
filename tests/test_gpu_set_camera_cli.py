"""The camera move at the two C++ front ends: `pt_render --orbit N` (one renderer, N views, pt_set_camera between them) and the
pathtrace.h shim with pathtraceSetKeepRenderer (pathtraceFree parks the renderer, the next pathtraceInit moves its camera)."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from camera_scenes import cornell_text, scene_path

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd")
BIN = os.path.join(PKG, "pt_render")
RES, SPP, FRAMES = (96, 54), 4, 4


def read_pfm(path):
    raw = open(path, "rb").read()
    head, dims, scale, body = raw.split(b"\n", 3)
    w, h = map(int, dims.split())
    assert head == b"PF" and float(scale) < 0
    return np.frombuffer(body, np.float32).reshape(h, w, 3)[::-1].reshape(-1, 3), w, h


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("devices", [None, "0,0"], ids=["single", "group"])
def test_orbit_frames_equal_fresh_renderers(tmp_path, devices):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path = scene_path(tmp_path, cornell_text, "A")
    plain = str(tmp_path / "plain")
    p = subprocess.run([BIN, path, "--spp", str(SPP), "--out", plain, "--pfm"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    out = str(tmp_path / "turn")
    cmd = [BIN, path, "--orbit", str(FRAMES), "--spp", str(SPP), "--res", f"{RES[0]}x{RES[1]}", "--out", out, "--pfm"]
    p = subprocess.run(cmd + (["--devices", devices] if devices else []), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert len(re.findall(r"^setup: tables \S+ ms, upload \S+ ms, buffers \S+ ms, probe \S+ ms$", p.stdout, re.M)) == 1
    lines = re.findall(r"^orbit: frame (\d+): camera (\S+) (\S+) (\S+), set_camera (\S+) ms, render (\S+) ms$", p.stdout, re.M)
    assert [int(m[0]) for m in lines] == list(range(FRAMES))
    assert float(lines[0][4]) == 0 and all(float(m[4]) > 0 for m in lines[1:])
    frames = []
    for f in range(FRAMES):
        base = f"{out}.{SPP}samp.orbit{f:03d}"
        assert os.path.exists(base + ".png")
        avg, w, h = read_pfm(base + ".pfm")
        assert (w, h) == RES
        frames.append(avg)
    assert np.array_equal(bits(frames[0]), bits(read_pfm(f"{plain}.{SPP}samp.pfm")[0]))  # frame 0: the scene's camera through init
    scene = capi.Scene(path)
    for f in range(1, FRAMES):
        cam = scene.orbit(np.float32(2 * math.pi / FRAMES), 0.0, 0.0)
        assert [float(np.float32(x)) for x in cam.position] == [float(np.float32(float(x))) for x in lines[f][1:4]]
        r = capi.Renderer(scene)
        try:
            r.render(1, SPP)
            img = r.readback()
        finally:
            r.free()
        assert np.array_equal(bits(img / np.float32(SPP)), bits(frames[f])), f
        assert not np.array_equal(bits(frames[f]), bits(frames[f - 1]))


@pytest.mark.parametrize("extra, named", [
    (["--features"], "--features"), (["--denoise"], "--denoise"), (["--denoise-guided"], "--denoise-guided"),
    (["--until-db", "30"], "--until-db"), (["--until-db", "30", "--adaptive", "0.5"], "--until-db"),
    (["--adaptive-threshold", "0.1"], "--adaptive-threshold"), (["--adaptive-threshold", "0.1", "--denoise-adaptive"], "--denoise-adaptive"),
    (["--convergence", "2"], "--convergence"), (["--gpus", "1", "--preview", "2"], "--preview"),
])
def test_orbit_refuses_what_it_does_not_carry_from_view_to_view(tmp_path, extra, named):
    path = scene_path(tmp_path, cornell_text, "A")
    p = subprocess.run([BIN, path, "--orbit", "4", "--spp", "4", "--out", str(tmp_path / "no")] + extra, capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and f"--orbit excludes {named} " in p.stderr, (p.returncode, p.stderr)
    assert not any(name.startswith("no.") for name in os.listdir(tmp_path))


def test_orbit_wants_a_frame_count(tmp_path):
    for bad in ("0", "1000", "x"):
        p = subprocess.run([BIN, scene_path(tmp_path, cornell_text, "A"), "--orbit", bad], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "--orbit wants the number of frames" in p.stderr


# ---- the shim ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/integration/keep_renderer_driver.cpp against include/pathtrace_amd.hpp, pt::Scene and the built library."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("shim") / "keep_renderer_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "integration", "keep_renderer_driver.cpp"),
           f"-I{ROOT}/include", f"-I{PKG}/csrc", f"-L{PKG}", "-lpt_amd", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def run_driver(driver, tmp_path, tag, keep, change):
    a, b = scene_path(tmp_path, cornell_text, "A"), scene_path(tmp_path, cornell_text, "B")
    out = str(tmp_path / tag)
    p = subprocess.run([driver, a, b, out, str(keep), str(change)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    calls = int(re.search(r"^set_camera_calls (\d+)$", p.stdout, re.M).group(1))
    return [open(f"{out}.{i}.f32", "rb").read() for i in range(2)], calls


@pytest.mark.parametrize("change", [0, 1], ids=["camera_only", "material_too"])
def test_shim_keeps_the_renderer_across_a_camera_move(driver, tmp_path, change):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    off, calls_off = run_driver(driver, tmp_path, "off", 0, change)
    on, calls_on = run_driver(driver, tmp_path, "on", 1, change)
    assert calls_off == 0
    assert calls_on == (0 if change else 1)  # another material: a real pt_free + pt_init
    assert len(off[0]) == RES[0] * RES[1] * 12 and on[0] == off[0] and on[1] == off[1] and on[1] != on[0]
    if not change:
        r = capi.Renderer(capi.Scene(scene_path(tmp_path, cornell_text, "B")))
        try:
            r.render(1, 4)
            assert r.readback().tobytes() == on[1]
        finally:
            r.free()
