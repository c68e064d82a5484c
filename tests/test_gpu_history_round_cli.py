"""`pt_render --orbit N --reproject [--denoise-history --history-moments] --history-extra G`: the history round at the command line
(pt_history_round between the lookup and the resolve), the files it writes and the line it prints per frame; its refusals; and the
same command without the option, whose files are those of the sequence without rounds."""
import os
import re
import subprocess

import numpy as np
import pytest

from camera_scenes import cornell_text, scene_path

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")
RES, SPP, FRAMES, G = (96, 54), 1, 3, 3  # a third of a turn per frame: little is carried, many pixels are fresh at every view
MOM = 2  # PT_HISTORY_MOMENTS
EXTS = (".pfm", ".reprojected.pfm", ".reprojected.denoised.pfm")


def read_pfm(path):
    raw = open(path, "rb").read()
    head, dims, scale, body = raw.split(b"\n", 3)
    w, h = map(int, dims.split())
    assert head == b"PF" and float(scale) < 0
    return np.frombuffer(body, np.float32).reshape(h, w, 3)[::-1].reshape(-1, 3)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(path, out, *extra):
    cmd = [BIN, path, "--orbit", str(FRAMES), "--reproject", "--spp", str(SPP), "--res", f"{RES[0]}x{RES[1]}", "--out", out, "--pfm", *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return p.stdout


def api_sequence(capi, path, moments, extra, min_history=0.0):
    """Per view (raw, blend[, filtered]) and (fresh, m) of the command's sequence through the API."""
    scene = capi.Scene(path, res=RES)
    r = capi.Renderer(scene)
    out = []
    try:
        for f in range(FRAMES):
            if f > 0:
                r.set_camera(scene.orbit(np.float32(2 * np.pi / FRAMES), 0.0, 0.0))
            first = f * (SPP + extra) + 1
            r.render(first, SPP)
            raw = r.readback() / np.float32(SPP)
            r.render_features(1, 1)
            if f > 0:
                r.history_reproject_ex(MOM if moments else 0)
            counts = r.history_round(first + SPP, extra, min_history) if extra else None
            images = [raw, r.history_resolve(SPP)] + ([r.history_denoise_ex(SPP, levels=3)] if moments else [])
            r.history_capture_ex(SPP, MOM if moments else 0)
            out.append((images, counts))
    finally:
        r.free()
    return out


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "alone"])
def test_history_extra_writes_the_api_s_pixels(tmp_path, moments):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path = scene_path(tmp_path, cornell_text, "A")
    out = str(tmp_path / "turn")
    filt = ["--denoise-history", "--history-moments", "--denoise-levels", "3"] if moments else []
    stdout = run(path, out, *filt, "--history-extra", str(G), "--history-min", "2.5")
    want = api_sequence(capi, path, moments, G, 2.5)
    lines = re.findall(r"^history: frame (\d+): (\d+) extra over (\d+) of (\d+) fresh pixels$", stdout, flags=re.M)
    assert [tuple(map(int, l)) for l in lines] == [(f, G, want[f][1][1], want[f][1][0]) for f in range(FRAMES)], stdout
    assert all(int(l[2]) > 0 for l in lines)
    assert f"then {G} more" in stdout
    for f in range(FRAMES):
        base = f"{out}.{SPP}samp.orbit{f:03d}"
        for ext, img in zip(EXTS, want[f][0]):
            assert np.array_equal(bits(read_pfm(base + ext)), bits(img)), (f, ext)
        assert os.path.exists(base + ".reprojected.denoised.pfm") == moments
    # the first view carries nothing, so without extras its blend would be the raw frame: the round's samples are in the written blend
    assert (bits(want[0][0][1]) != bits(want[0][0][0])).any()


def test_without_the_option_nothing_changes(tmp_path):
    """The command without --history-extra: no line about extras, the iteration numbers f spp + 1 .., and the files of the sequence
    without rounds (tests/test_gpu_history_moments_cli.py's, which the counted kernels never touch: E stays absent)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path = scene_path(tmp_path, cornell_text, "A")
    out = str(tmp_path / "turn")
    stdout = run(path, out, "--denoise-history", "--history-moments", "--denoise-levels", "3")
    assert "extra" not in stdout and "(f + 1) * 1" in stdout
    want = api_sequence(capi, path, True, 0)
    for f in range(FRAMES):
        base = f"{out}.{SPP}samp.orbit{f:03d}"
        for ext, img in zip(EXTS, want[f][0]):
            assert np.array_equal(bits(read_pfm(base + ext)), bits(img)), (f, ext)


@pytest.mark.parametrize("extra, named", [
    (["--orbit", "3", "--reproject", "--denoise-history", "--history-extra", "3", "--spp", "2"], "--history-extra excludes --denoise-history without --history-moments"),
    (["--orbit", "3", "--history-extra", "3"], "--history-extra wants --orbit N --reproject"),
    (["--history-extra", "3"], "--history-extra wants --orbit N --reproject"),
    (["--orbit", "3", "--reproject", "--history-min", "2"], "--history-min and --history-extra-cap go with --history-extra"),
    (["--orbit", "3", "--reproject", "--history-extra", "0"], "--history-extra wants the iterations"),
    (["--orbit", "3", "--reproject", "--history-extra", "3", "--history-extra-cap", "1.5"], "--history-extra-cap wants"),
])
def test_refusals(tmp_path, extra, named):
    path = scene_path(tmp_path, cornell_text, "A")
    p = subprocess.run([BIN, path, "--out", str(tmp_path / "x")] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and named in p.stderr, (p.returncode, p.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("x.")]
