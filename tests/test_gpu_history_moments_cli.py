"""`pt_render --orbit N --reproject --denoise-history --history-moments`: the blend of every view filtered with the variance the
history's moments give (pt_history_*_ex with PT_HISTORY_MOMENTS, pt_history_denoise_ex) at the command line, at 1 spp per view."""
import os
import subprocess

import numpy as np
import pytest

from camera_scenes import cornell_text, scene_path

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")
RES, SPP, FRAMES = (96, 54), 1, 3  # a third of a turn per frame: little is carried, every path of the code is taken
MOM = 2  # PT_HISTORY_MOMENTS


def read_pfm(path):
    raw = open(path, "rb").read()
    head, dims, scale, body = raw.split(b"\n", 3)
    w, h = map(int, dims.split())
    assert head == b"PF" and float(scale) < 0
    return np.frombuffer(body, np.float32).reshape(h, w, 3)[::-1].reshape(-1, 3), w, h


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_orbit_history_moments_at_1_spp_writes_the_api_s_pixels(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path = scene_path(tmp_path, cornell_text, "A")
    out = str(tmp_path / "turn")
    cmd = [BIN, path, "--orbit", str(FRAMES), "--reproject", "--denoise-history", "--history-moments", "--denoise-levels", "3", "--spp", str(SPP),
           "--res", f"{RES[0]}x{RES[1]}", "--out", out, "--pfm"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    files = []
    for f in range(FRAMES):
        base = f"{out}.{SPP}samp.orbit{f:03d}"
        for ext in (".png", ".pfm", ".reprojected.png", ".reprojected.pfm", ".reprojected.denoised.png", ".reprojected.denoised.pfm"):
            assert os.path.exists(base + ext), base + ext
        files.append((read_pfm(base + ".pfm")[0], read_pfm(base + ".reprojected.pfm")[0], read_pfm(base + ".reprojected.denoised.pfm")[0]))
    # the same sequence through the API: one render call per view and no fold, features, the lookup with moments, resolve, the filter,
    # the capture with moments, the move
    scene = capi.Scene(path, res=RES)
    r = capi.Renderer(scene)
    try:
        for f in range(FRAMES):
            if f > 0:
                r.set_camera(scene.orbit(np.float32(2 * np.pi / FRAMES), 0.0, 0.0))
            r.render(f * SPP + 1, SPP)
            r.render_features(1, 1)
            if f > 0:
                r.history_reproject_ex(MOM)
            raw, blend, filtered = r.readback() / np.float32(SPP), r.history_resolve(SPP), r.history_denoise_ex(SPP, levels=3)
            r.history_capture_ex(SPP, MOM)
            for got, want, name in zip(files[f], (raw, blend, filtered), ("raw", "reprojected", "reprojected.denoised")):
                assert np.array_equal(bits(got), bits(want)), (f, name)
            assert (bits(filtered) != bits(blend)).any()
    finally:
        r.free()


@pytest.mark.parametrize("extra, named", [
    (["--orbit", "3", "--reproject", "--history-moments"], "--history-moments wants --denoise-history"),
    (["--history-moments"], "--history-moments wants --denoise-history"),
    (["--orbit", "3", "--history-moments", "--denoise-history"], "--denoise-history wants --orbit N --reproject"),
    (["--orbit", "3", "--reproject", "--denoise-history", "--spp", "1"], "--denoise-history wants at least 2 iterations"),  # without it: as before
    (["--orbit", "3", "--reproject", "--denoise-history", "--history-moments", "--gpus", "1"], "--gpus / --devices"),
])
def test_refusals(tmp_path, extra, named):
    path = scene_path(tmp_path, cornell_text, "A")
    p = subprocess.run([BIN, path, "--spp", "2", "--out", str(tmp_path / "x")] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and named in p.stderr, (p.returncode, p.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("x.")]
