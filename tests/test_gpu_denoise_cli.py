"""`pt_render --denoise`: the .denoised.pfm next to the image equals Renderer.denoise of the same run, bit for bit, through the
single-context path and through a group of two contexts; bad values of the flags end with exit status 1."""
import os
import subprocess

import numpy as np
import pytest

from denoise_ref import bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")


def read_pfm(path):
    raw = open(path, "rb").read()
    head, dims, scale, body = raw.split(b"\n", 3)
    w, h = map(int, dims.split())
    assert head == b"PF" and float(scale) < 0
    return np.frombuffer(body, np.float32).reshape(h, w, 3)[::-1].reshape(-1, 3), w, h


@pytest.fixture(scope="module")
def expected(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(64, 48)), aa_jitter=True)
    try:
        r.render(1, 3)
        r.render_features(1, 3)
        return dict(default=r.denoise(3), custom=r.denoise(3, levels=2, sigma_color=2.0, sigma_normal=-1.0, sigma_position=0.5, keep_albedo=True))
    finally:
        r.free()


@pytest.mark.parametrize("extra,which", [([], "default"), (["--devices", "0,0"], "default"),
                                         (["--denoise-levels", "2", "--denoise-sigma", "2,-1,0.5", "--denoise-keep-albedo"], "custom")])
def test_pt_render_denoise_files(scene_dir, tmp_path, expected, extra, which):
    assert os.path.exists(BIN), "pt_render not built"
    out = str(tmp_path / "X")
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "64x48", "--spp", "3", "--aa", "--denoise", "--pfm", "--out", out] + extra,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    for name in ("png", "pfm", "denoised.png", "denoised.pfm", "normal.pfm"):  # --denoise implies --features
        assert os.path.exists(f"{out}.3samp.{name}"), name
    got, w, h = read_pfm(f"{out}.3samp.denoised.pfm")
    assert (w, h) == (64, 48)
    assert np.array_equal(bits(got), bits(expected[which]))
    raw, _, _ = read_pfm(f"{out}.3samp.pfm")
    assert (bits(got) != bits(raw)).any()


@pytest.mark.parametrize("args", [["--denoise", "--denoise-levels", "9"], ["--denoise", "--denoise-levels", "0"], ["--denoise", "--denoise-levels", "x"],
                                  ["--denoise", "--denoise-sigma", "1,2"], ["--denoise", "--denoise-sigma", "1,2,nan"], ["--denoise-levels", "3"]])
def test_bad_values_exit_1(scene_dir, tmp_path, args):
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "16x12", "--spp", "1", "--out", str(tmp_path / "X")] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "denoise" in p.stderr, (p.returncode, p.stderr)
    assert not os.path.exists(str(tmp_path / "X") + ".1samp.png")  # refused before anything is rendered


def test_usage_names_the_flag():
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode == 1 and "--denoise" in p.stdout
