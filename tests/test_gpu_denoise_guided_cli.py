"""`pt_render --denoise-guided`: the .denoised.pfm next to the image equals Renderer.denoise_guided of the same renders and folds,
bit for bit, through the single-context path, a group of two contexts and after --until-db; the two refusals end with status 1."""
import os
import re
import subprocess

import numpy as np
import pytest

from denoise_ref import bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")
RES, SPP = (64, 48), 8


def read_pfm(path):
    raw = open(path, "rb").read()
    head, dims, scale, body = raw.split(b"\n", 3)
    w, h = map(int, dims.split())
    assert head == b"PF" and float(scale) < 0
    return np.frombuffer(body, np.float32).reshape(h, w, 3)[::-1].reshape(-1, 3), w, h


def guided(scene_dir, sizes, **opts):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=RES), aa_jitter=True)
    try:
        first = 1
        for n in sizes:
            r.render(first, n)
            r.noise_fold()
            first += n
        r.render_features(1, first - 1)
        return r.denoise_guided(**opts)
    finally:
        r.free()


@pytest.fixture(scope="module")
def expected(scene_dir):
    return dict(default=guided(scene_dir, [2, 2, 2, 2]), threes=guided(scene_dir, [3, 3, 2]),
                custom=guided(scene_dir, [2, 2, 2, 2], levels=2, sigma_color=4.0, sigma_normal=-1.0, sigma_position=0.5, keep_albedo=True))


@pytest.mark.parametrize("extra,which", [([], "default"), (["--devices", "0,0"], "default"), (["--until-group", "3"], "threes"),
                                         (["--denoise-levels", "2", "--denoise-sigma", "4,-1,0.5", "--denoise-keep-albedo"], "custom")])
def test_pt_render_denoise_guided_files(scene_dir, tmp_path, expected, extra, which):
    assert os.path.exists(BIN), "pt_render not built"
    out = str(tmp_path / "X")
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "%dx%d" % RES, "--spp", str(SPP), "--aa", "--denoise-guided", "--pfm", "--out", out] + extra,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    for name in ("png", "pfm", "denoised.png", "denoised.pfm", "normal.pfm"):  # --denoise-guided implies --features
        assert os.path.exists(f"{out}.{SPP}samp.{name}"), name
    got, w, h = read_pfm(f"{out}.{SPP}samp.denoised.pfm")
    assert (w, h) == RES
    assert np.array_equal(bits(got), bits(expected[which]))
    raw, _, _ = read_pfm(f"{out}.{SPP}samp.pfm")
    assert (bits(got) != bits(raw)).any()


@pytest.mark.parametrize("extra", [[], ["--devices", "0,0"]])
def test_after_until_db(scene_dir, tmp_path, expected, extra):
    """A target no render reaches: --until-db renders the cap in groups of 2 and --denoise-guided filters what it left."""
    out = str(tmp_path / "X")
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "%dx%d" % RES, "--spp", str(SPP), "--aa", "--denoise-guided", "--pfm", "--out", out,
                        "--until-db", "99", "--until-group", "2"] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert re.search(r"^noise: 8 iterations, 4 groups, estimated PSNR \S+ dB$", p.stdout, re.M), p.stdout
    got, _, _ = read_pfm(f"{out}.{SPP}samp.denoised.pfm")
    assert np.array_equal(bits(got), bits(expected["default"]))


@pytest.mark.parametrize("args,word", [(["--denoise-guided", "--spp", "1"], "at least 2"), (["--denoise-guided", "--denoise", "--spp", "4"], "exclude")])
def test_refusals_exit_1(scene_dir, tmp_path, args, word):
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "16x12", "--out", str(tmp_path / "X")] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "--denoise-guided" in p.stderr and word in p.stderr, (p.returncode, p.stderr)
    assert not os.listdir(tmp_path)  # refused before anything is rendered


def test_usage_names_the_flag():
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode == 1 and "--denoise-guided" in p.stdout
