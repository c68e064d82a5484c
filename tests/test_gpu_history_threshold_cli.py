"""`pt_render --orbit N --reproject --denoise-history --history-threshold E`: every view renders two uniform groups and then rounds over
the pixels whose blend with the carried history is above the threshold (pt_history_render_threshold), and is resolved, filtered and
captured by every pixel's own count, at the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

from camera_scenes import cornell_text, scene_path

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")
RES, CAP, GROUP, FRAMES, E, FRACTION, MIN_PIXELS = (96, 54), 12, 2, 3, 0.25, 0.5, 3
LINE = re.compile(r"^threshold: frame (\d+): (\d+) iterations, (\d+) rounds, (\d+) samples \((\S+) of uniform\), (-?\d+) pixels above, "
                  r"estimated PSNR of the blend (\S+) dB$", re.M)
EXTS = (".png", ".pfm", ".reprojected.png", ".reprojected.pfm", ".reprojected.denoised.png", ".reprojected.denoised.pfm")


def read_pfm(path):
    raw = open(path, "rb").read()
    head, dims, scale, body = raw.split(b"\n", 3)
    w, h = map(int, dims.split())
    assert head == b"PF" and float(scale) < 0
    return np.frombuffer(body, np.float32).reshape(h, w, 3)[::-1].reshape(-1, 3)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def orbit_cmd(path, out, *more):
    return [BIN, path, "--orbit", str(FRAMES), "--reproject", "--denoise-history", "--spp", str(CAP), "--res", f"{RES[0]}x{RES[1]}", "--out", out, "--pfm", *more]


def test_orbit_by_threshold_prints_its_lines_and_writes_the_api_s_pixels(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path = scene_path(tmp_path, cornell_text, "A")
    out = str(tmp_path / "turn")
    p = subprocess.run(orbit_cmd(path, out, "--history-threshold", str(E), "--history-threshold-cap", str(FRACTION), "--history-threshold-min-pixels",
                                 str(MIN_PIXELS), "--history-threshold-group", str(GROUP)), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = LINE.findall(p.stdout)
    assert [int(l[0]) for l in lines] == list(range(FRAMES)), p.stdout
    files = []
    for f in range(FRAMES):
        base = f"{out}.{CAP}samp.orbit{f:03d}"  # --spp is the cap, and what the names carry
        for ext in EXTS:
            assert os.path.exists(base + ext), base + ext
        files.append((read_pfm(base + ".pfm"), read_pfm(base + ".reprojected.pfm"), read_pfm(base + ".reprojected.denoised.pfm")))
    # the same sequence through the API: features, the lookup, the driver, resolve, the filter, the estimate, the capture, the move
    scene = capi.Scene(path, res=RES)
    n = RES[0] * RES[1]
    r = capi.Renderer(scene)
    try:
        for f in range(FRAMES):
            if f > 0:
                r.set_camera(scene.orbit(np.float32(2 * np.pi / FRAMES), 0.0, 0.0))
            r.render_features(1, 1)
            if f > 0:
                r.history_reproject_ex()
            done, samples, above = r.history_render_threshold(f * CAP + 1, CAP, E, FRACTION, GROUP, MIN_PIXELS)
            rounds = r.noise()["groups"] - 2
            raw, blend, filtered = r.resolve(), r.history_resolve_adaptive(), r.history_denoise_adaptive()
            psnr = capi.psnr_from_sse(r.history_noise_adaptive(), n)
            r.history_capture_adaptive()
            assert (int(lines[f][1]), int(lines[f][2]), int(lines[f][3]), int(lines[f][5])) == (done, rounds, samples, above), (f, lines[f])
            assert abs(float(lines[f][4]) - samples / (CAP * n)) < 1e-4 and np.float32(lines[f][6]) == np.float32(psnr)
            assert done == 2 * GROUP + rounds * GROUP and (above <= MIN_PIXELS or done == CAP)
            for got, want, name in zip(files[f], (raw, blend, filtered), ("raw", "reprojected", "reprojected.denoised")):
                assert np.array_equal(bits(got), bits(want)), (f, name)
    finally:
        r.free()
    assert int(lines[0][2]) >= 1 and int(lines[0][3]) < CAP * n  # rounds ran, over a part of the frame


def test_without_the_option_every_file_is_what_the_old_calls_give(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path = scene_path(tmp_path, cornell_text, "A")
    outs = [str(tmp_path / "plain"), str(tmp_path / "again")]
    for out in outs:
        p = subprocess.run(orbit_cmd(path, out), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and "threshold:" not in p.stdout, (p.stdout, p.stderr)
    scene = capi.Scene(path, res=RES)
    group = (CAP + 3) // 4
    r = capi.Renderer(scene)
    try:
        for f in range(FRAMES):
            base = [f"{out}.{CAP}samp.orbit{f:03d}" for out in outs]
            for ext in EXTS:
                assert open(base[0] + ext, "rb").read() == open(base[1] + ext, "rb").read(), ext
            if f > 0:
                r.set_camera(scene.orbit(np.float32(2 * np.pi / FRAMES), 0.0, 0.0))
            for done in range(0, CAP, group):
                r.render(f * CAP + 1 + done, min(group, CAP - done))
                r.noise_fold()
            r.render_features(1, 1)
            if f > 0:
                r.history_reproject_ex()
            want = (r.readback() / np.float32(CAP), r.history_resolve(CAP), r.history_denoise(CAP))
            r.history_capture_ex(CAP)
            for ext, img in zip((".pfm", ".reprojected.pfm", ".reprojected.denoised.pfm"), want):
                assert np.array_equal(bits(read_pfm(base[0] + ext)), bits(img)), (f, ext)
    finally:
        r.free()


HISTORY = ["--orbit", "3", "--reproject", "--denoise-history"]
THR = ["--history-threshold", "0.1"]


@pytest.mark.parametrize("extra, named", [
    (["--orbit", "3", "--reproject"] + THR, "--history-threshold wants --orbit N --reproject --denoise-history"),
    (THR, "--history-threshold wants --orbit N --reproject --denoise-history"),
    (HISTORY + THR + ["--history-until-db", "30"], "--history-threshold excludes --history-until-db"),
    (HISTORY + THR + ["--history-moments"], "--history-threshold excludes --history-moments"),
    (HISTORY + THR + ["--history-extra", "2"], "--history-threshold excludes --history-extra"),
    (["--orbit", "3", "--orbit-still", "--move", "1:0.1,0,0"] + HISTORY[2:] + THR + ["--history-probe"], "--history-threshold excludes --history-probe"),
    (HISTORY + THR + ["--history-moments", "--history-feedback"], "--history-threshold excludes --history-feedback"),
    (HISTORY + THR + ["--gpus", "1"], "--history-threshold excludes --gpus / --devices"),
    (HISTORY + THR + ["--devices", "0"], "--history-threshold excludes --gpus / --devices"),
    (HISTORY + ["--history-threshold", "-0.5"], "--history-threshold wants"),
    (HISTORY + ["--history-threshold", "inf"], "--history-threshold wants"),
    (HISTORY + ["--history-threshold", "nan"], "--history-threshold wants"),
    (HISTORY + THR + ["--history-threshold-cap", "0"], "--history-threshold-cap wants"),
    (HISTORY + THR + ["--history-threshold-cap", "1.5"], "--history-threshold-cap wants"),
    (HISTORY + THR + ["--history-threshold-min-pixels", "-1"], "--history-threshold-min-pixels wants"),
    (HISTORY + THR + ["--history-threshold-group", "-1"], "--history-threshold-group wants"),
    (HISTORY + ["--history-threshold-cap", "0.5"], "--history-threshold-cap wants --history-threshold"),
    (HISTORY + ["--history-threshold-min-pixels", "2"], "--history-threshold-min-pixels wants --history-threshold"),
    (HISTORY + ["--history-threshold-group", "2"], "--history-threshold-group wants --history-threshold"),
])
def test_refusals(tmp_path, extra, named):
    path = scene_path(tmp_path, cornell_text, "A")
    p = subprocess.run([BIN, path, "--spp", "4", "--out", str(tmp_path / "x")] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and named in p.stderr, (p.returncode, p.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("x.")]
