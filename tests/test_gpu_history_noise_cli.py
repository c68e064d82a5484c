"""`pt_render --orbit N --reproject --denoise-history --history-until-db X`: every view renders until the estimated PSNR of the blend
with the carried history is above X (pt_history_render_until) at the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

from camera_scenes import cornell_text, scene_path

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")
RES, CAP, GROUP, FRAMES, TARGET = (32, 24), 12, 2, 4, 22.0
LINE = re.compile(r"^until: frame (\d+): (\d+) iterations, (\d+) groups, estimated PSNR of the blend (\S+) dB \(the view alone (\S+) dB\)$", re.M)


def read_pfm(path):
    raw = open(path, "rb").read()
    head, dims, scale, body = raw.split(b"\n", 3)
    w, h = map(int, dims.split())
    assert head == b"PF" and float(scale) < 0
    return np.frombuffer(body, np.float32).reshape(h, w, 3)[::-1].reshape(-1, 3), w, h


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_orbit_until_prints_its_lines_and_writes_the_api_s_pixels(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path = scene_path(tmp_path, cornell_text, "A")
    out = str(tmp_path / "turn")
    cmd = [BIN, path, "--orbit", str(FRAMES), "--reproject", "--denoise-history", "--history-until-db", str(TARGET), "--history-until-group", str(GROUP),
           "--spp", str(CAP), "--res", f"{RES[0]}x{RES[1]}", "--out", out, "--pfm"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = LINE.findall(p.stdout)
    assert [int(l[0]) for l in lines] == list(range(FRAMES)), p.stdout
    files = []
    for f in range(FRAMES):
        base = f"{out}.{CAP}samp.orbit{f:03d}"  # --spp is the cap, and what the names carry
        for ext in (".png", ".pfm", ".reprojected.png", ".reprojected.pfm", ".reprojected.denoised.png", ".reprojected.denoised.pfm"):
            assert os.path.exists(base + ext), base + ext
        files.append((read_pfm(base + ".pfm")[0], read_pfm(base + ".reprojected.pfm")[0], read_pfm(base + ".reprojected.denoised.pfm")[0]))
    # the same sequence through the API: features, the lookup, the driver, resolve, the filter, the capture, the move
    scene = capi.Scene(path, res=RES)
    r = capi.Renderer(scene)
    try:
        for f in range(FRAMES):
            if f > 0:
                r.set_camera(scene.orbit(np.float32(2 * np.pi / FRAMES), 0.0, 0.0))
            r.render_features(1, 1)
            if f > 0:
                r.history_reproject_ex()
            done, psnr, view = r.history_render_until(f * CAP + 1, CAP, TARGET, GROUP)
            groups = r.noise()["groups"]
            assert (int(lines[f][1]), int(lines[f][2])) == (done, groups) and done % GROUP == 0 and groups == done // GROUP >= 2
            assert np.float32(lines[f][3]) == np.float32(psnr) and np.float32(lines[f][4]) == np.float32(view)
            assert psnr > TARGET or done == CAP
            raw, blend, filtered = r.readback() / np.float32(done), r.history_resolve(done), r.history_denoise(done)
            r.history_capture_ex(done)
            for got, want, name in zip(files[f], (raw, blend, filtered), ("raw", "reprojected", "reprojected.denoised")):
                assert np.array_equal(bits(got), bits(want)), (f, name)
    finally:
        r.free()
    assert int(lines[0][1]) > 2 * GROUP  # the first view has its own samples only; the target is not met at the floor of two folds


def test_without_the_option_nothing_changes(tmp_path):
    path = scene_path(tmp_path, cornell_text, "A")
    cmd = [BIN, path, "--orbit", "2", "--reproject", "--denoise-history", "--spp", "4", "--res", f"{RES[0]}x{RES[1]}", "--out", str(tmp_path / "plain")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "until:" not in p.stdout, (p.stdout, p.stderr)


HISTORY = ["--orbit", "3", "--reproject", "--denoise-history"]


@pytest.mark.parametrize("extra, named", [
    (["--orbit", "3", "--reproject", "--history-until-db", "30"], "--history-until-db wants --orbit N --reproject --denoise-history"),
    (["--history-until-db", "30"], "--history-until-db wants --orbit N --reproject --denoise-history"),
    (HISTORY + ["--history-until-db", "30", "--history-moments"], "--history-until-db excludes --history-moments"),
    (["--orbit", "3", "--reproject", "--denoise-history", "--history-until-db", "30", "--history-extra", "2"], "--history-until-db excludes --history-extra"),
    (["--orbit", "3", "--orbit-still", "--move", "1:0.1,0,0"] + HISTORY[2:] + ["--history-until-db", "30", "--history-probe"], "--history-until-db excludes --history-probe"),
    (HISTORY + ["--history-until-db", "30", "--history-moments", "--history-feedback"], "--history-until-db excludes --history-feedback"),
    (HISTORY + ["--history-until-db", "inf"], "--history-until-db wants"),
    (HISTORY + ["--history-until-db", "nan"], "--history-until-db wants"),
    (HISTORY + ["--history-until-db", "30", "--history-until-group", "-1"], "--history-until-group wants"),
    (HISTORY + ["--history-until-group", "2"], "--history-until-group wants --history-until-db"),
    (["--orbit", "3", "--until-db", "30"], "--orbit excludes --until-db"),
])
def test_refusals(tmp_path, extra, named):
    path = scene_path(tmp_path, cornell_text, "A")
    p = subprocess.run([BIN, path, "--spp", "4", "--out", str(tmp_path / "x")] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and named in p.stderr, (p.returncode, p.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("x.")]
