"""`pt_render --adaptive-threshold E [--adaptive-cap F] [--adaptive-min-pixels P]`: the printed line, the file name
(ceil(samples / pixels)) and the PFM, which holds the resolved image of Renderer.render_threshold + resolve bit for bit; what the
flag excludes ends with exit status 1 before anything is rendered."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")
RES, CAP, GROUP, THRESHOLD, MIN_PIXELS = (64, 48), 60, 4, 0.08, 5
N = RES[0] * RES[1]
LINE = (r"^adaptive: threshold (\S+): (\d+) iterations, (\d+) rounds, (\d+) samples \((\S+) of uniform\), (\d+) pixels above, "
        r"estimated PSNR (\S+) dB$")


def expected(scene_dir, **kw):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=RES), aa_jitter=True)
    try:
        done, samples, above = r.render_threshold(1, CAP, THRESHOLD, group_iters=GROUP, **kw)
        noise = r.noise()
        return done, samples, above, noise["groups"], capi.psnr_from_sse(noise["sse"], N), r.resolve()
    finally:
        r.free()


@pytest.mark.parametrize("flags, kw", [([], {}), (["--adaptive-cap", "0.1", "--adaptive-min-pixels", str(MIN_PIXELS)], dict(max_fraction=0.1, min_pixels=MIN_PIXELS))],
                         ids=["defaults", "cap-and-floor"])
def test_pt_render_adaptive_threshold(scene_dir, tmp_path, flags, kw):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    assert os.path.exists(BIN), "pt_render not built"
    done, samples, above, groups, psnr, resolved = expected(scene_dir, **kw)
    assert 2 * GROUP < done <= CAP and groups > 2 and 2 * GROUP * N < samples < done * N  # some rounds ran, over part of the frame
    out = str(tmp_path / "X")
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "%dx%d" % RES, "--spp", str(CAP), "--aa", "--pfm", "--out", out, "--adaptive-threshold", str(THRESHOLD),
                        "--until-group", str(GROUP)] + flags, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    m = re.search(LINE, p.stdout, re.M)
    assert m, p.stdout
    assert np.float32(m.group(1)) == np.float32(THRESHOLD)
    assert (int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(6))) == (done, groups - 2, samples, above), (m.groups(), done, groups, samples, above)
    assert abs(float(m.group(5)) - samples / (done * N)) < 1e-4
    assert np.float32(m.group(7)) == np.float32(psnr), (m.group(7), psnr)
    if kw:
        assert above <= MIN_PIXELS or done == CAP
    spp = -(-samples // N)
    assert spp < done
    for name in ("png", "pfm"):
        assert os.path.exists(f"{out}.{spp}samp.{name}"), (name, os.listdir(tmp_path))
    assert f"{spp} spp" in p.stdout  # the timing line speaks of the samples, not of the iteration numbers
    got = capi.load_pfm(f"{out}.{spp}samp.pfm").reshape(-1, 3)
    assert np.array_equal(got.view(np.uint32), resolved.view(np.uint32))


def test_takes_denoise_adaptive(scene_dir, tmp_path):
    out = str(tmp_path / "X")
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "%dx%d" % RES, "--spp", "24", "--out", out, "--adaptive-threshold", str(THRESHOLD), "--until-group",
                        str(GROUP), "--denoise-adaptive"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and re.search(LINE, p.stdout, re.M), (p.stdout, p.stderr)
    assert any(f.endswith(".denoised.png") for f in os.listdir(tmp_path)), os.listdir(tmp_path)


EXCLUDES, WANTS_THRESHOLD, WANTS_NUMBER = "--adaptive-threshold excludes", "want --adaptive-threshold", "--adaptive-threshold wants"
T = ["--adaptive-threshold", "0.05"]


@pytest.mark.parametrize("args, message", [(T + ["--until-db", "30", "--adaptive", "0.25"], EXCLUDES), (T + ["--until-db", "30"], EXCLUDES),
                                           (T + ["--gpus", "1"], EXCLUDES), (T + ["--devices", "0,0"], EXCLUDES), (T + ["--denoise"], EXCLUDES),
                                           (T + ["--denoise-guided"], EXCLUDES), (T + ["--convergence", "2"], EXCLUDES),
                                           (T + ["--reference", "nowhere.pfm"], EXCLUDES), (T + ["--preview", "2"], EXCLUDES),
                                           (["--adaptive-cap", "0.5"], WANTS_THRESHOLD), (["--adaptive-min-pixels", "3"], WANTS_THRESHOLD),
                                           (["--adaptive-threshold", "-1"], WANTS_NUMBER), (["--adaptive-threshold", "nan"], WANTS_NUMBER),
                                           (["--adaptive-threshold", "x"], WANTS_NUMBER), (T + ["--adaptive-cap", "0"], "--adaptive-cap wants"),
                                           (T + ["--adaptive-cap", "1.5"], "--adaptive-cap wants"), (T + ["--adaptive-min-pixels", "-2"], "--adaptive-min-pixels wants")])
def test_exclusions_exit_1(scene_dir, tmp_path, args, message):
    """The driver's own refusal, by its message: an unknown flag would exit 1 too."""
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "16x12", "--spp", "8", "--out", str(tmp_path / "X")] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and message in p.stderr and "unknown argument" not in p.stderr, (p.returncode, p.stderr)
    assert not os.listdir(tmp_path)  # refused before anything is rendered


def test_usage_names_the_flags():
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode == 1 and all(f in p.stdout for f in ("--adaptive-threshold", "--adaptive-cap", "--adaptive-min-pixels"))
