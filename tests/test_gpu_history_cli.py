"""`pt_render --orbit N --reproject`: the image carried from view to view at the command line (pt_history_*)."""
import os
import re
import subprocess

import numpy as np
import pytest

from camera_scenes import cornell_text, scene_path

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")
RES, SPP, FRAMES = (96, 54), 4, 36  # a full turn in steps of 10 degrees; the first three frames are looked at


def read_pfm(path):
    raw = open(path, "rb").read()
    head, dims, scale, body = raw.split(b"\n", 3)
    w, h = map(int, dims.split())
    assert head == b"PF" and float(scale) < 0
    return np.frombuffer(body, np.float32).reshape(h, w, 3)[::-1].reshape(-1, 3), w, h


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_orbit_reproject_writes_the_files(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path = scene_path(tmp_path, cornell_text, "A")
    out = str(tmp_path / "turn")
    cmd = [BIN, path, "--orbit", str(FRAMES), "--reproject", "--spp", str(SPP), "--res", f"{RES[0]}x{RES[1]}", "--out", out, "--pfm"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert len(re.findall(r"^history: frame f renders iterations f \* 4 \+ 1 \.\. \(f \+ 1\) \* 4, not 1 \.\. 4", p.stdout, re.M)) == 1
    lines = re.findall(r"^history: frame (\d+): (\d+) of (\d+) pixels carried, mean weight (\S+)$", p.stdout, re.M)
    assert [int(m[0]) for m in lines] == list(range(FRAMES)) and all(int(m[2]) == RES[0] * RES[1] for m in lines)
    assert int(lines[0][1]) == 0 and float(lines[0][3]) == 0
    raw, carried = [], []
    for f in range(FRAMES):
        base = f"{out}.{SPP}samp.orbit{f:03d}"
        for ext in (".png", ".pfm", ".reprojected.png", ".reprojected.pfm"):
            assert os.path.exists(base + ext), base + ext
        if f < 3:
            raw.append(read_pfm(base + ".pfm")[0])
            img, w, h = read_pfm(base + ".reprojected.pfm")
            assert (w, h) == RES
            carried.append(img)
    # frame 0 has no history: its reprojected image is its raw one, pixels and bytes
    assert np.array_equal(bits(carried[0]), bits(raw[0]))
    assert open(f"{out}.{SPP}samp.orbit000.reprojected.png", "rb").read() == open(f"{out}.{SPP}samp.orbit000.png", "rb").read()
    for f in range(1, 3):
        n = int(lines[f][1])
        assert 0 < n < RES[0] * RES[1] and SPP <= float(lines[f][3]) <= 32
        differ = int((bits(carried[f]) != bits(raw[f])).any(axis=1).sum())
        assert n // 2 < differ <= n, (f, differ, n)
    assert float(lines[1][3]) == SPP and float(lines[2][3]) > SPP and max(float(m[3]) for m in lines) > 8  # the weights add up from view to view
    # frame f renders iterations f * spp + 1 ...: frame 1's raw image is a fresh renderer's at the moved camera with iterations 5 .. 8
    scene = capi.Scene(path, res=RES)
    cam = scene.orbit(np.float32(2 * np.pi / FRAMES), 0.0, 0.0)
    r = capi.Renderer(scene)
    try:
        r.render(SPP + 1, SPP)
        img = r.readback()
    finally:
        r.free()
    assert np.array_equal(bits(img / np.float32(SPP)), bits(raw[1])), cam.position[:]


def test_history_cap_is_passed_on(tmp_path):
    path = scene_path(tmp_path, cornell_text, "A")
    cmd = [BIN, path, "--orbit", str(FRAMES), "--reproject", "--history-cap", "5", "--spp", str(SPP), "--res", "48x27", "--out", str(tmp_path / "cap5")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    weights = [float(m) for m in re.findall(r"^history: frame \d+: \d+ of \d+ pixels carried, mean weight (\S+)$", p.stdout, re.M)]
    assert len(weights) == FRAMES and weights[1] == SPP and 4.5 < max(weights) <= 5.0


@pytest.mark.parametrize("extra, named", [
    (["--orbit", "3", "--reproject", "--gpus", "1"], "--gpus / --devices"),
    (["--orbit", "3", "--reproject", "--devices", "0,0"], "--gpus / --devices"),
    (["--reproject"], "--orbit"),
    (["--orbit", "3", "--history-cap", "8"], "--reproject"),
    (["--orbit", "3", "--reproject", "--history-cap", "0"], "--history-cap"),
    (["--orbit", "3", "--reproject", "--history-cap", "-2"], "--history-cap"),
])
def test_refusals(tmp_path, extra, named):
    path = scene_path(tmp_path, cornell_text, "A")
    p = subprocess.run([BIN, path, "--spp", "2", "--out", str(tmp_path / "x")] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and named in p.stderr, (p.returncode, p.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("x.")]
