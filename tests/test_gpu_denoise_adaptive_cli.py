"""`pt_render --adaptive F --denoise-adaptive`: the filtered PFM, which holds Renderer.render_adaptive + render_features +
denoise_adaptive bit for bit, beside the outputs `--adaptive` writes anyway; the flag it needs and the flags it excludes end with
exit status 1 before anything is rendered."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")
RES, CAP, GROUP, FRACTION = (64, 48), 30, 4, 0.25  # test_gpu_adaptive_cli.py's run
N = RES[0] * RES[1]
ADAPTIVE_LINE = r"^adaptive: (\d+) iterations, (\d+) rounds, (\d+) samples \((\S+) of uniform\), estimated PSNR (\S+) dB$"


@pytest.fixture(scope="module")
def expected(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=RES), aa_jitter=True)
    try:
        done, samples, psnr = r.render_adaptive(1, CAP, target_db=99.0, fraction=FRACTION, group_iters=GROUP)
        groups, resolved = r.noise()["groups"], r.resolve()
        r.render_features(1, done)
        return done, samples, psnr, groups, resolved, r.denoise_adaptive(), r.denoise_adaptive(levels=3, sigma_color=2.0, keep_albedo=True)
    finally:
        r.free()


@pytest.mark.parametrize("options", [[], ["--denoise-levels", "3", "--denoise-sigma", "2,0,0", "--denoise-keep-albedo"]], ids=["defaults", "options"])
def test_pt_render_denoise_adaptive(scene_dir, tmp_path, expected, options):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    assert os.path.exists(BIN), "pt_render not built"
    done, samples, psnr, groups, resolved, filtered, filtered_options = expected
    out = str(tmp_path / "X")
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "%dx%d" % RES, "--spp", str(CAP), "--aa", "--pfm", "--out", out, "--until-db", "99",
                        "--until-group", str(GROUP), "--adaptive", str(FRACTION), "--denoise-adaptive"] + options, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    m = re.search(ADAPTIVE_LINE, p.stdout, re.M)  # the line --adaptive prints, unchanged
    assert m, p.stdout
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (done, groups - 2, samples)
    assert np.float32(m.group(5)) == np.float32(psnr), (m.group(5), psnr)
    base = f"{out}.{-(-samples // N)}samp"
    for name in ("png", "pfm", "denoised.png", "denoised.pfm", "normal.pfm", "albedo.pfm", "position.pfm", "depth.pfm"):
        assert os.path.exists(f"{base}.{name}"), (name, os.listdir(tmp_path))
    assert f"Saved {base}.denoised.pfm." in p.stdout
    assert np.array_equal(capi.load_pfm(f"{base}.pfm").reshape(-1, 3).view(np.uint32), resolved.view(np.uint32))
    got = capi.load_pfm(f"{base}.denoised.pfm").reshape(-1, 3)
    want = filtered_options if options else filtered
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (filtered.view(np.uint32) != resolved.view(np.uint32)).any() and (filtered.view(np.uint32) != filtered_options.view(np.uint32)).any()


ADAPTIVE = ["--until-db", "30", "--adaptive", "0.25"]


@pytest.mark.parametrize("args, message", [(["--denoise-adaptive"], "--denoise-adaptive wants --adaptive"),
                                           (["--until-db", "30", "--denoise-adaptive"], "--denoise-adaptive wants --adaptive"),
                                           (ADAPTIVE + ["--denoise-adaptive", "--denoise"], "--denoise-adaptive excludes"),
                                           (ADAPTIVE + ["--denoise-adaptive", "--denoise-guided"], "--denoise-adaptive excludes"),
                                           (["--denoise-adaptive", "--denoise"], "--denoise-adaptive excludes")])
def test_needs_and_exclusions_exit_1(scene_dir, tmp_path, args, message):
    """The driver's own refusal, by its message: an unknown flag would exit 1 too."""
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "16x12", "--spp", "8", "--out", str(tmp_path / "X")] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and message in p.stderr and "unknown argument" not in p.stderr, (p.returncode, p.stderr)
    assert not os.listdir(tmp_path)  # refused before anything is rendered


def test_usage_names_the_flag():
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode == 1 and "--denoise-adaptive" in p.stdout
