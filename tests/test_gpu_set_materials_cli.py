"""`pt_render --orbit N [--orbit-still] (--recolor M:DR,DG,DB | --emit M:DE) [--move ..] [--reproject [--history-probe]]` on the device:
the refusals of the new options, the `material:` lines and the files of a run against the same calls through the API."""
import os
import re
import subprocess

import numpy as np
import pytest

import history_materials_ref as mref
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
WALL, LIGHT = 2, 0


@pytest.fixture(scope="module")
def sphere_path(tmp_path_factory):
    return mot.sim_scene_paths(tmp_path_factory.mktemp("gpu_set_materials_cli"), frames=1)[0]


def read_pfm(path):
    raw = open(path, "rb").read()
    head, dims, scale, body = raw.split(b"\n", 3)
    w, h = map(int, dims.split())
    assert head == b"PF" and float(scale) < 0
    return np.frombuffer(body, np.float32).reshape(h, w, 3)[::-1].reshape(-1, 3)


def api_frames(sphere_path, recolor, emit, move, still, probe):
    """The command line's calls through the API: per frame (raw average, blend, the check's counts, the edited material)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(sphere_path, res=href.RES)
    r = capi.Renderer(scene)
    out = []
    flags = mref.MATERIALS | (mot.MOTION if move else 0)
    try:
        for f in range(FRAMES):
            if f > 0:
                if move:
                    trs = scene.geom_trs(mot.SPHERE)
                    trs[0] += f32(0.5)
                    scene.set_geom_trs(mot.SPHERE, trs)
                    r.set_geoms(scene)
                if recolor:
                    m = scene.material(WALL)
                    m.color[:] = [float(f32(c) + f32(d)) for c, d in zip(m.color, recolor)]
                    scene.set_material(WALL, m)
                if emit:
                    m = scene.material(LIGHT)
                    m.emittance = float(f32(m.emittance) + f32(emit))
                    scene.set_material(LIGHT, m)
                r.set_materials(scene)
                if not still:
                    r.set_camera(scene.orbit(f32(2 * np.pi / FRAMES), 0.0, 0.0))
            r.render(f * SPP + 1, SPP)
            raw = r.readback() / f32(SPP)
            r.render_features(1, 1)
            counts = (0, 0, 0)
            if f > 0:
                r.history_reproject_ex(flags)
                if probe:
                    counts = r.history_probe_check()
            if probe:
                r.history_probe_keep(f * SPP + 1, SPP, f % 9)
            out.append((raw, r.history_resolve(SPP), counts, scene.material(WALL if recolor else LIGHT)))
            r.history_capture(SPP)
    finally:
        r.free()
    return out


@pytest.mark.parametrize("recolor,emit,move,still,probe", [((-0.25, 0.0, 0.25), 0.0, False, False, False), (None, -0.375, False, True, True),
                                                           ((-0.25, 0.0, 0.25), -0.375, True, True, False)], ids=["recolor-orbit", "emit-still-probe", "both-move-still"])
def test_cli_equals_the_api_sequence(tmp_path, sphere_path, recolor, emit, move, still, probe):
    out = str(tmp_path / "edited")
    cmd = [BIN, sphere_path, "--orbit", str(FRAMES), "--spp", str(SPP), "--res", f"{W}x{H}", "--out", out, "--pfm", "--reproject"]
    cmd += (["--recolor", f"{WALL}:" + ",".join(str(x) for x in recolor)] if recolor else []) + (["--emit", f"{LIGHT}:{emit}"] if emit else [])
    cmd += (["--move", MOVE] if move else []) + (["--orbit-still"] if still else []) + (["--history-probe"] if probe else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    want = api_frames(sphere_path, recolor, emit, move, still, probe)
    lines = re.findall(r"^material: frame (\d+): material (\d+) colour (\S+) (\S+) (\S+) emittance (\S+), set_materials (\S+) ms$", p.stdout, re.M)
    per_frame = (1 if recolor else 0) + (1 if emit else 0)
    assert len(lines) == per_frame * (FRAMES - 1), p.stdout
    first = [ln for ln in lines if int(ln[1]) == (WALL if recolor else LIGHT)]
    for (f, _, cr, cg, cb, e, ms), (_, _, _, m) in zip(first, want[1:]):
        assert np.array_equal(bits(np.array([cr, cg, cb, e], f32)), bits(np.array(list(m.color) + [m.emittance], f32))) and float(ms) > 0, f
    assert [int(ln[0]) for ln in first] == list(range(1, FRAMES))
    if probe:
        probes = re.findall(r"^probe: frame (\d+): (\d+) of (\d+) probes changed, (\d+) skipped$", p.stdout, re.M)
        assert [tuple(map(int, m)) for m in probes] == [(f, c[1], c[0], c[2]) for f, (_, _, c, _) in enumerate(want)]
        assert all(c[1] > 0 for _, _, c, _ in want[1:])  # a dimmed light changes every probe with a sample that ended on it
    cams = re.findall(r"^orbit: frame \d+: camera (\S+ \S+ \S+),", p.stdout, re.M)
    assert len(set(cams)) == (1 if still else FRAMES)
    for f, (raw, blend, _, _) in enumerate(want):
        base = f"{out}.{SPP}samp.orbit{f:03d}"
        assert np.array_equal(bits(read_pfm(base + ".pfm")), bits(raw)), f
        assert np.array_equal(bits(read_pfm(base + ".reprojected.pfm")), bits(blend)), f


def test_cli_with_a_group(tmp_path, sphere_path):
    """--devices 0,0: pt_group_set_materials over two contexts; the frames are the single renderer's."""
    outs = {}
    for name, extra in (("one", []), ("two", ["--devices", "0,0"])):
        out = str(tmp_path / name)
        p = subprocess.run([BIN, sphere_path, "--orbit", "2", "--spp", str(SPP), "--res", f"{W}x{H}", "--out", out, "--pfm", "--emit", f"{LIGHT}:-0.5"] + extra,
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and len(re.findall(r"^material: frame 1: material 0 colour 1 1 1 emittance 1, set_materials", p.stdout, re.M)) == 1, (p.stdout, p.stderr)
        outs[name] = [read_pfm(f"{out}.{SPP}samp.orbit{f:03d}.pfm") for f in range(2)]
    for a, b in zip(outs["one"], outs["two"]):
        assert np.array_equal(bits(a), bits(b))
    assert not np.array_equal(bits(outs["one"][0]), bits(outs["one"][1]))


@pytest.mark.parametrize("extra, named", [
    (["--recolor", "2:0.1,0,0"], "--recolor goes with --orbit"),
    (["--emit", "0:0.5"], "--emit goes with --orbit"),
    (["--orbit", "3", "--recolor", "5:0.1,0,0"], "--recolor: material 5 is outside the scene's 5 materials"),
    (["--orbit", "3", "--emit", "9:1"], "--emit: material 9 is outside the scene's 5 materials"),
    (["--orbit", "3", "--recolor", "2:0.1,inf,0"], "--recolor wants M:DR,DG,DB"),
    (["--orbit", "3", "--recolor", "2:0.1,0"], "--recolor wants M:DR,DG,DB"),
    (["--orbit", "3", "--emit", "0:nan"], "--emit wants M:DE"),
    (["--orbit", "3", "--emit", "0:-0.1", "--reproject", "--denoise-history", "--history-moments", "--history-feedback"], "--emit excludes --history-feedback"),
    (["--orbit", "3", "--recolor", "2:0.1,0,0", "--reproject", "--denoise-history", "--history-moments", "--history-feedback"], "--recolor excludes --history-feedback"),
    # the next two are refused with these texts before this feature too: they pin that the widened conditions keep the old wording
    (["--orbit", "3", "--orbit-still"], "--orbit-still wants --orbit N --move"),
    (["--orbit", "3", "--reproject", "--history-probe"], "--history-probe wants --move"),
    (["--orbit", "3", "--emit", "0:-0.1", "--reproject", "--history-probe"], "--history-probe wants --orbit-still"),
])
def test_cli_refusals(tmp_path, sphere_path, extra, named):
    p = subprocess.run([BIN, sphere_path, "--spp", "2", "--out", str(tmp_path / "x")] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and named in p.stderr, (p.returncode, p.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("x.")]
