"""`pt_render --orbit N --reproject --denoise-history --history-moments --history-feedback`: the filtered image fed back into the
history at the command line (pt_history_*_ex with PT_HISTORY_FEEDBACK, pt_history_denoise_feedback), at 1 spp per view, with
--history-extra and --move composed in (the camera stands still and the sphere moves, so that nearly every pixel carries); and the same
command without the option, which writes what it wrote."""
import os
import subprocess

import numpy as np
import pytest

import history_motion_ref as mot
from camera_scenes import cornell_text, scene_path

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")
RES, SPP, FRAMES, EXTRA = (96, 54), 1, 3, 3
MOM, MOTION, FB = 2, 4, 16  # PT_HISTORY_MOMENTS, PT_HISTORY_MOTION, PT_HISTORY_FEEDBACK
MOVE = f"{mot.SPHERE}:0.5,0,0"


@pytest.fixture(scope="module")
def sphere_path(tmp_path_factory):
    return mot.sim_scene_paths(tmp_path_factory.mktemp("gpu_history_feedback_cli"), frames=1)[0]
EXTS = (".png", ".pfm", ".reprojected.png", ".reprojected.pfm", ".reprojected.denoised.png", ".reprojected.denoised.pfm")


def read_pfm(path):
    raw = open(path, "rb").read()
    head, dims, scale, body = raw.split(b"\n", 3)
    w, h = map(int, dims.split())
    assert head == b"PF" and float(scale) < 0
    return np.frombuffer(body, np.float32).reshape(h, w, 3)[::-1].reshape(-1, 3), w, h


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(path, out, *more):
    cmd = [BIN, path, "--orbit", str(FRAMES), "--reproject", "--denoise-history", "--history-moments", "--denoise-levels", "3", "--spp", str(SPP),
           "--history-extra", str(EXTRA), "--orbit-still", "--move", MOVE, "--res", f"{RES[0]}x{RES[1]}", "--out", out, "--pfm", *more]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return p.stdout


def api_sequence(capi, path, feedback, **fb):
    """(raw, blend, filtered) per view through the API, in the command line's order: move, render, features, lookup, round, resolve,
    filter, capture."""
    scene = capi.Scene(path, res=RES)
    r = capi.Renderer(scene)
    flags = MOM | (FB if feedback else 0)
    out = []
    try:
        for f in range(FRAMES):
            if f > 0:
                trs = scene.geom_trs(mot.SPHERE)
                trs[0] += np.float32(0.5)
                scene.set_geom_trs(mot.SPHERE, trs)
                r.set_geoms(scene)
            first = f * (SPP + EXTRA) + 1
            r.render(first, SPP)
            raw = r.readback() / np.float32(SPP)
            r.render_features(1, 1)
            if f > 0:
                r.history_reproject_ex(flags | MOTION)
            r.history_round(first + SPP, EXTRA)
            blend = r.history_resolve(SPP)
            filtered = r.history_denoise_feedback(SPP, levels=3, **fb) if feedback else r.history_denoise_ex(SPP, levels=3)
            r.history_capture_ex(SPP, flags)
            out.append((raw, blend, filtered))
    finally:
        r.free()
    return out


def test_the_option_writes_the_same_names_and_the_api_s_pixels(tmp_path, sphere_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path = sphere_path
    without, with_fb = str(tmp_path / "without"), str(tmp_path / "with")
    plain_out = run(path, without)
    fb_out = run(path, with_fb, "--history-feedback", "--feedback-level", "2", "--feedback-variance", "0")
    assert "feedback: the output of filter level 2 is fed back, variance rule 0" in fb_out
    assert "feedback" not in plain_out
    strip = lambda text, tag: [ln.replace(tag, "X") for ln in text.splitlines() if ln.startswith(("history:", "Saved "))]  # noqa: E731
    assert strip(plain_out, without) == strip(fb_out, with_fb) and len(strip(plain_out, without)) == 1 + FRAMES * (2 + len(EXTS))  # (one line says how the iterations are numbered)
    # (the history's lines and the files' are the same; the one new line is the feedback's; the others carry times)
    assert [ln for ln in fb_out.splitlines() if ln.startswith("feedback:")] == ["feedback: the output of filter level 2 is fed back, variance rule 0"]
    names = sorted(os.path.basename(p)[len("without"):] for p in os.listdir(tmp_path) if os.path.basename(p).startswith("without."))
    assert names == sorted(os.path.basename(p)[len("with"):] for p in os.listdir(tmp_path) if os.path.basename(p).startswith("with."))
    assert len(names) == FRAMES * len(EXTS)
    want_plain, want_fb = api_sequence(capi, path, False), api_sequence(capi, path, True, level=2, variance=0)
    for f in range(FRAMES):
        a, b = (f"{o}.{SPP}samp.orbit{f:03d}" for o in (without, with_fb))
        for ext in EXTS:
            assert os.path.exists(a + ext) and os.path.exists(b + ext), ext
        # without the option: what the command wrote before — the moments sequence's pixels
        for ext, want in zip((".pfm", ".reprojected.pfm", ".reprojected.denoised.pfm"), want_plain[f]):
            assert np.array_equal(bits(read_pfm(a + ext)[0]), bits(want)), (f, ext, "without")
        # with it: the raw frame and the blend are bytewise the same files; the filtered image is the feedback sequence's
        for ext in (".png", ".pfm", ".reprojected.png", ".reprojected.pfm"):
            assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), (f, ext)
        assert np.array_equal(bits(read_pfm(b + ".reprojected.denoised.pfm")[0]), bits(want_fb[f][2])), (f, "with")
        same_filtered = open(a + ".reprojected.denoised.pfm", "rb").read() == open(b + ".reprojected.denoised.pfm", "rb").read()
        assert same_filtered == (f == 0)  # the first view has no history to differ in


def test_the_defaults_are_printed(tmp_path, sphere_path):
    out = run(sphere_path, str(tmp_path / "d"), "--history-feedback")
    assert "feedback: the output of filter level 1 is fed back, variance rule 1" in out


@pytest.mark.parametrize("extra, named", [
    (["--orbit", "3", "--reproject", "--denoise-history", "--history-feedback"], "--history-feedback wants --history-moments"),
    (["--history-feedback"], "--history-feedback wants --history-moments"),
    (["--orbit", "3", "--reproject", "--denoise-history", "--history-moments", "--feedback-level", "2"], "want --history-feedback"),
    (["--orbit", "3", "--reproject", "--denoise-history", "--history-moments", "--history-feedback", "--feedback-level", "0"], "--feedback-level wants"),
    (["--orbit", "3", "--reproject", "--denoise-history", "--history-moments", "--history-feedback", "--feedback-variance", "2"], "--feedback-variance wants"),
])
def test_refusals(tmp_path, extra, named):
    path = scene_path(tmp_path, cornell_text, "A")
    p = subprocess.run([BIN, path, "--spp", "2", "--out", str(tmp_path / "x")] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and named in p.stderr, (p.returncode, p.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("x.")]


def test_a_level_beyond_the_filter_s_is_refused_by_the_library(tmp_path):
    path = scene_path(tmp_path, cornell_text, "A")
    p = subprocess.run([BIN, path, "--orbit", "2", "--reproject", "--denoise-history", "--history-moments", "--history-feedback", "--feedback-level", "4",
                        "--denoise-levels", "3", "--spp", "1", "--res", "32x24", "--out", str(tmp_path / "y")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "pt_history_denoise_feedback: feedback level 4 is not in 1 .. 3" in p.stderr, (p.returncode, p.stderr)
