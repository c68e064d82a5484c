"""`pt_render --adaptive F --until-db X`: the printed line, the file name (ceil(samples / pixels)) and the PFM, which holds the
resolved image of Renderer.render_adaptive + resolve bit for bit; the flags it needs and excludes end with exit status 1 before
anything is rendered."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")
RES, CAP, GROUP, FRACTION = (64, 48), 30, 4, 0.25  # the cap cuts the last round to 2 iterations
N = RES[0] * RES[1]


@pytest.fixture(scope="module")
def expected(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=RES), aa_jitter=True)
    try:
        done, samples, psnr = r.render_adaptive(1, CAP, target_db=99.0, fraction=FRACTION, group_iters=GROUP)
        return done, samples, psnr, r.noise()["groups"], r.resolve()
    finally:
        r.free()


def test_pt_render_adaptive(scene_dir, tmp_path, expected):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    assert os.path.exists(BIN), "pt_render not built"
    done, samples, psnr, groups, resolved = expected
    m_pixels = -(-N // 4)
    assert done == CAP and groups == 8 and samples == 2 * GROUP * N + (5 * GROUP + 2) * m_pixels
    out = str(tmp_path / "X")
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "%dx%d" % RES, "--spp", str(CAP), "--aa", "--pfm", "--out", out, "--until-db", "99",
                        "--until-group", str(GROUP), "--adaptive", str(FRACTION)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    m = re.search(r"^adaptive: (\d+) iterations, (\d+) rounds, (\d+) samples \((\S+) of uniform\), estimated PSNR (\S+) dB$", p.stdout, re.M)
    assert m, p.stdout
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (done, groups - 2, samples)
    assert abs(float(m.group(4)) - samples / (done * N)) < 1e-4
    assert np.float32(m.group(5)) == np.float32(psnr), (m.group(5), psnr)
    spp = -(-samples // N)
    assert spp < CAP
    for name in ("png", "pfm"):
        assert os.path.exists(f"{out}.{spp}samp.{name}"), (name, os.listdir(tmp_path))
    assert f"{spp} spp" in p.stdout  # the timing line speaks of the samples, not of the iteration numbers
    got = capi.load_pfm(f"{out}.{spp}samp.pfm").reshape(-1, 3)
    assert np.array_equal(got.view(np.uint32), resolved.view(np.uint32))


NEEDS, FRACTION_MSG, EXCLUDES = "--adaptive wants --until-db", "--adaptive wants the fraction", "--adaptive excludes"


@pytest.mark.parametrize("args, message", [(["--adaptive", "0.25"], NEEDS), (["--until-db", "30", "--adaptive", "0"], FRACTION_MSG),
                                           (["--until-db", "30", "--adaptive", "1.5"], FRACTION_MSG), (["--until-db", "30", "--adaptive", "x"], FRACTION_MSG),
                                           (["--until-db", "30", "--adaptive", "0.25", "--gpus", "1"], EXCLUDES),
                                           (["--until-db", "30", "--adaptive", "0.25", "--devices", "0,0"], EXCLUDES),
                                           (["--until-db", "30", "--adaptive", "0.25", "--denoise"], EXCLUDES),
                                           (["--until-db", "30", "--adaptive", "0.25", "--denoise-guided"], EXCLUDES),
                                           (["--until-db", "30", "--adaptive", "0.25", "--convergence", "2"], EXCLUDES),
                                           (["--until-db", "30", "--adaptive", "0.25", "--reference", "nowhere.pfm"], EXCLUDES),
                                           (["--until-db", "30", "--adaptive", "0.25", "--preview", "2"], EXCLUDES)])
def test_needs_and_exclusions_exit_1(scene_dir, tmp_path, args, message):
    """The driver's own refusal, by its message: an unknown flag would exit 1 too."""
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "16x12", "--spp", "8", "--out", str(tmp_path / "X")] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and message in p.stderr and "unknown argument" not in p.stderr, (p.returncode, p.stderr)
    assert not os.listdir(tmp_path)  # refused before anything is rendered


def test_usage_names_the_flag():
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode == 1 and "--adaptive" in p.stdout
