"""`pt_render --features`: the four PFM files next to the image equal the C ABI's feature buffers divided by the sample
count, bit for bit, through the single-context path and through a group of two contexts."""
import os
import subprocess

import numpy as np
import pytest

from features_ref import bits

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
        r.render_features(1, 3)
        f = r.readback_features()
    finally:
        r.free()
    three = np.float32(3)
    return dict(normal=f["normal"] / three, albedo=f["albedo"] / three, position=f["position"] / three,
                depth=np.repeat((f["depth"] / three)[:, None], 3, axis=1))


@pytest.mark.parametrize("extra", [[], ["--devices", "0,0"]])
def test_pt_render_features_files(scene_dir, tmp_path, expected, extra):
    assert os.path.exists(BIN), "pt_render not built"
    out = str(tmp_path / "X")
    p = subprocess.run([BIN, scene_dir["cornell"], "--res", "64x48", "--spp", "3", "--aa", "--features", "--out", out] + extra,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert os.path.exists(f"{out}.3samp.png")
    assert (expected["depth"] > 0).any() and (expected["depth"] == 0).any()
    for name, want in expected.items():
        got, w, h = read_pfm(f"{out}.3samp.{name}.pfm")
        assert (w, h) == (64, 48)
        assert np.array_equal(bits(got), bits(want)), name


def test_usage_names_the_flag():
    p = subprocess.run([BIN], capture_output=True, text=True)
    assert p.returncode == 1 and "--features" in p.stdout
