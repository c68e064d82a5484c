"""`pt_render --until-db`: the render stops by its own noise estimate below the --spp cap, the file name carries the iterations
actually rendered and the printed estimate is Renderer.render_until's, through the single-context path and through a group of two
contexts; bad values of the flags end with exit status 1 before anything is rendered."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")
RES, CAP, GROUP = (64, 48), 40, 4


@pytest.fixture(scope="module")
def expected(scene_dir):
    """(target, iterations, groups, estimated PSNR) of Renderer.render_until for a target between the fourth and fifth group."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = RES[0] * RES[1]
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=RES), aa_jitter=True)
    try:
        db = []
        for M in range(1, 6):
            r.render(1 + GROUP * (M - 1), GROUP)
            r.noise_fold()
            db.append(capi.psnr_from_sse(r.noise()["sse"], n) if M >= 2 else -1.0)
        target = round(0.5 * (db[3] + db[4]), 3)
        assert max(db[:4]) < target < db[4], (db, target)
        r.clear()
        done, psnr = r.render_until(1, CAP, target, group_iters=GROUP)
        return target, done, r.noise()["groups"], psnr
    finally:
        r.free()


@pytest.mark.parametrize("extra", [[], ["--devices", "0,0"]])
def test_pt_render_until_db(scene_dir, tmp_path, expected, extra):
    assert os.path.exists(BIN), "pt_render not built"
    target, done, groups, psnr = expected
    assert done == 5 * GROUP < CAP
    out = str(tmp_path / "X")
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "%dx%d" % RES, "--spp", str(CAP), "--aa", "--pfm", "--out", out, "--until-db", repr(target),
                        "--until-group", str(GROUP)] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    m = re.search(r"^noise: (\d+) iterations, (\d+) groups, estimated PSNR (\S+) dB$", p.stdout, re.M)
    assert m, p.stdout
    assert (int(m.group(1)), int(m.group(2))) == (done, groups)
    if extra:  # the group adds two contexts' sums: the last bits may differ
        assert abs(float(m.group(3)) - psnr) < 1e-3
    else:
        assert np.float32(m.group(3)) == np.float32(psnr), (m.group(3), psnr)
    for name in ("png", "pfm"):
        assert os.path.exists(f"{out}.{done}samp.{name}"), (name, os.listdir(tmp_path))
    assert not os.path.exists(f"{out}.{CAP}samp.png")
    assert f"{done} spp" in p.stdout


def test_cap_reached(scene_dir, tmp_path):
    out = str(tmp_path / "X")
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "32x24", "--spp", "5", "--aa", "--out", out, "--until-db", "99", "--until-group", "2"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert re.search(r"^noise: 5 iterations, 3 groups, estimated PSNR \S+ dB$", p.stdout, re.M), p.stdout
    assert os.path.exists(out + ".5samp.png")


@pytest.mark.parametrize("args", [["--until-db", "nan"], ["--until-db", "inf"], ["--until-db", "x"], ["--until-db", "30", "--until-group", "-1"],
                                  ["--until-db", "30", "--until-group", "x"], ["--until-group", "4"], ["--until-db", "30", "--gpus", "1", "--preview", "2"]])
def test_bad_values_exit_1(scene_dir, tmp_path, args):
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "16x12", "--spp", "1", "--out", str(tmp_path / "X")] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "--until" in p.stderr, (p.returncode, p.stderr)
    assert not os.listdir(tmp_path)  # refused before anything is rendered


def test_usage_names_the_flag():
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode == 1 and "--until-db" in p.stdout and "--until-group" in p.stdout
