"""`pt_render --orbit N --orbit-still --move G:DX,DY,DZ --reproject --history-probe [--probe-radius R] [--probe-gain X]` on the device:
the refusals of the new options, the `probe:` lines and the files of a run against the same calls through the API, and a run without
the options, whose output has no new line and whose files are those of the calls it made before."""
import os
import re
import subprocess

import numpy as np
import pytest

import history_motion_ref as mot
import history_ref as href
from history_ref import bits, f32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")
W, H = href.RES
SPP = href.SPP
FRAMES = 3
MOVE = f"{mot.SPHERE}:0.5,0,0"


@pytest.fixture(scope="module")
def sphere_path(tmp_path_factory):
    return mot.sim_scene_paths(tmp_path_factory.mktemp("gpu_history_probe_cli"), frames=1)[0]


def read_pfm(path):
    raw = open(path, "rb").read()
    head, dims, scale, body = raw.split(b"\n", 3)
    w, h = map(int, dims.split())
    assert head == b"PF" and float(scale) < 0
    return np.frombuffer(body, np.float32).reshape(h, w, 3)[::-1].reshape(-1, 3)


def run(sphere_path, out, extra):
    cmd = [BIN, sphere_path, "--orbit", str(FRAMES), "--move", MOVE, "--spp", str(SPP), "--res", f"{W}x{H}", "--out", out, "--pfm", "--reproject"] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return p.stdout


def api_frames(sphere_path, still, probe, **opts):
    """The command line's calls through the API: per frame (raw average, blend, the check's counts)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(sphere_path, res=href.RES)
    r = capi.Renderer(scene)
    out = []
    try:
        for f in range(FRAMES):
            if f > 0:
                trs = scene.geom_trs(mot.SPHERE)
                trs[0] += f32(0.5)
                scene.set_geom_trs(mot.SPHERE, trs)
                r.set_geoms(scene)
                if not still:
                    r.set_camera(scene.orbit(f32(2 * np.pi / FRAMES), 0.0, 0.0))
            r.render(f * SPP + 1, SPP)
            raw = r.readback() / f32(SPP)
            r.render_features(1, 1)
            counts = (0, 0, 0)
            if f > 0:
                r.history_reproject_ex(mot.MOTION)
                if probe:
                    counts = r.history_probe_check(**opts)
            if probe:
                r.history_probe_keep(f * SPP + 1, SPP, f % 9)
            out.append((raw, r.history_resolve(SPP), counts))
            r.history_capture(SPP)
    finally:
        r.free()
    return out


@pytest.mark.parametrize("extra,opts", [([], {}), (["--probe-radius", "1", "--probe-gain", "1"], dict(radius=1, gain=1.0)),
                                        (["--probe-radius", "0", "--probe-gain", "0.5"], dict(radius=-1, gain=0.5))], ids=["defaults", "r1g1", "r0g0.5"])
def test_cli_probe_equals_the_api_sequence(tmp_path, sphere_path, extra, opts):
    out = str(tmp_path / "probed")
    stdout = run(sphere_path, out, ["--orbit-still", "--history-probe"] + extra)
    want = api_frames(sphere_path, True, True, **opts)
    lines = re.findall(r"^probe: frame (\d+): (\d+) of (\d+) probes changed, (\d+) skipped$", stdout, re.M)
    assert [tuple(map(int, m)) for m in lines] == [(f, c[1], c[0], c[2]) for f, (_, _, c) in enumerate(want)]
    assert want[0][2] == (0, 0, 0) and all(c[0] == 32 * 18 and c[1] > 0 for _, _, c in want[1:])
    cams = re.findall(r"^orbit: frame \d+: camera (\S+ \S+ \S+),", stdout, re.M)
    assert len(cams) == FRAMES and len(set(cams)) == 1  # the camera stands still
    for f, (raw, blend, _) in enumerate(want):
        base = f"{out}.{SPP}samp.orbit{f:03d}"
        assert os.path.exists(base + ".png") and os.path.exists(base + ".reprojected.png")
        assert np.array_equal(bits(read_pfm(base + ".pfm")), bits(raw)), f
        assert np.array_equal(bits(read_pfm(base + ".reprojected.pfm")), bits(blend)), f


@pytest.mark.parametrize("still", [False, True], ids=["orbit", "orbit-still"])
def test_cli_without_the_probes_is_what_it_was(tmp_path, sphere_path, still):
    """No `probe:` line, the files of before, and the images of the calls the command made before (--orbit-still only leaves the camera
    where it is)."""
    out = str(tmp_path / "plain")
    stdout = run(sphere_path, out, ["--orbit-still"] if still else [])
    assert not re.search(r"^probe:", stdout, re.M)
    kinds = [ln.split(":")[0] for ln in stdout.splitlines() if not ln.startswith("Saved")]
    per_frame = ["orbit", "history"]
    assert kinds == ["setup", "history"] + per_frame + (["move"] + per_frame) * (FRAMES - 1), kinds
    want = api_frames(sphere_path, still, False)
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(f"plain.{SPP}samp.orbit{f:03d}{kind}" for f in range(FRAMES) for kind in (".png", ".pfm", ".reprojected.png", ".reprojected.pfm"))
    for f, (raw, blend, _) in enumerate(want):
        base = f"{out}.{SPP}samp.orbit{f:03d}"
        assert np.array_equal(bits(read_pfm(base + ".pfm")), bits(raw)), f
        assert np.array_equal(bits(read_pfm(base + ".reprojected.pfm")), bits(blend)), f
    cams = re.findall(r"^orbit: frame \d+: camera (\S+ \S+ \S+),", stdout, re.M)
    assert len(set(cams)) == (1 if still else FRAMES)


@pytest.mark.parametrize("extra, named", [
    (["--orbit", "3", "--orbit-still"], "--orbit-still wants --orbit N --move"),
    (["--orbit-still", "--move", MOVE], "--move goes with --orbit"),
    (["--orbit", "3", "--reproject", "--history-probe"], "--history-probe wants --move"),
    (["--orbit", "3", "--move", MOVE, "--reproject", "--history-probe"], "--history-probe wants --orbit-still"),
    (["--orbit", "3", "--move", MOVE, "--orbit-still", "--history-probe"], "--history-probe wants --reproject"),
    (["--orbit", "3", "--move", MOVE, "--orbit-still", "--reproject", "--probe-radius", "1"], "--probe-radius and --probe-gain go with --history-probe"),
    (["--orbit", "3", "--move", MOVE, "--orbit-still", "--reproject", "--history-probe", "--probe-radius", "5"], "--probe-radius wants"),
    (["--orbit", "3", "--move", MOVE, "--orbit-still", "--reproject", "--history-probe", "--probe-gain", "-1"], "--probe-gain wants"),
    (["--orbit", "3", "--move", MOVE, "--orbit-still", "--reproject", "--history-probe", "--probe-gain", "nan"], "--probe-gain wants"),
])
def test_cli_refusals(tmp_path, sphere_path, extra, named):
    p = subprocess.run([BIN, sphere_path, "--spp", "2", "--out", str(tmp_path / "x")] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and named in p.stderr, (p.returncode, p.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("x.")]
