"""boxIntersectionTest / sphereIntersectionTest per ray in every arithmetic mode against float64 (tests/prim_ref64.py), through
pt_stage_intersect, which runs the mode's own geom_test (csrc/pt_arith.inc: in fast the symmetric cube test with clamped
reciprocals and the normal code from the sign of r, the single-FMA sphere discriminant, getPointOnRay without renormalisation).

tests/test_gpu_traversal_consistency.py and tests/test_gpu_grid_rays.py show that the hierarchy returns what the leaf tests return;
this shows that the leaf tests are right.  On the CLEAR rays (prim_ref64: every comparison of the float64 test at least a relative
1e-4 from its boundary) of three scenes — cornell, random_scene_text(11, 20) with 26 rotated, non-uniformly scaled leaves, and
random_scene_text(1, 3) — and seven ray families, the bounce family among them (origins 0.001 off a surface, half of the
directions within 2 degrees of the tangent plane: what depths >= 1 trace):
  hit / miss and the material equal float64's; a cube's normal is the table entry, bit for bit; a sphere's normal is on float64's
  side and within 4 x the geom's yardstick of it; t and the point are within 4 x the geom's yardstick — the ORACLE's own maximum
  distance from float64 on that geom's clear hits, measured on the CPU and pinned in prim_ref64.YARDSTICK (4: 1-ulp
  approximations against 0.5-ulp correct rounding; the fast forms add at most as many roundings again).
On the other rays everything is finite and nothing more is asserted.  `exact` goes first and equals the oracle bit for bit on every
ray, which anchors rays, scenes and restatement on the device."""
import numpy as np
import pytest

import prim_ref64 as p64
from cosc_4397_pathtracing_raytracing_project_amd import capi, scenes

pytestmark = pytest.mark.gpu
MODES = ("exact", "fma", "fast")
FACTOR = 4.0


@pytest.fixture(scope="module")
def prepared(tmp_path_factory):
    """Per scene, built once and left unchanged: the scene, its rays, float64's verdict, the oracle's hits."""
    from oracle import binding as ob
    made = {}

    def get(name):
        if name not in made:
            path = scenes.write_scene(p64.scene_text(name), str(tmp_path_factory.mktemp("prim_modes") / f"{name}.txt"))
            sc = capi.Scene(path)
            G = p64.geoms(sc.geoms())
            rays = p64.ray_set(name, G)
            ob.set_math_mode(ob.PORTABLE)
            ob.load_scene(path)
            orc = ob.intersect(rays["o"], rays["d"])
            ob.set_math_mode(ob.LIBM)
            made[name] = dict(scene=sc, G=G, rays=rays, ref=p64.intersect(G, rays["o"], rays["d"]), table=p64.cube_normal_table(G), oracle=orc)
        return made[name]
    return get


def subset(d: dict, idx) -> dict:
    return {k: (np.ascontiguousarray(v[..., idx]) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def check(arith, what, P, idx, got):
    ref, orc = subset(P["ref"], idx), subset(P["oracle"], idx)
    for k in ("t", "nrm", "pt"):
        assert np.isfinite(got[k]).all(), f"{what} {k}: {int((~np.isfinite(got[k])).sum())} values are not finite"
    if arith == "exact":
        for k in ("t", "mat", "nrm", "pt"):
            same = np.ascontiguousarray(got[k]).view(np.uint32) == np.ascontiguousarray(orc[k]).view(np.uint32)
            assert same.all(), (what, k, np.argwhere(~same)[:8].tolist())
    m = p64.measure_against(P["G"], ref, got, P["table"])
    o, d = P["rays"]["o"][:, idx], P["rays"]["d"][:, idx]
    describe = lambda i: f"ray {int(idx[i])}: o {o[:, i].tolist()} d {d[:, i].tolist()} float64 geom {int(ref['geom'][i])} t {float(ref['t'][i])} gap {float(ref['gap'][i]):.3g}; got t {float(got['t'][i])} mat {int(got['mat'][i])} nrm {got['nrm'][:, i].tolist()}"
    for k in ("hit_bad", "mat_bad", "cube_nrm_bad", "sphere_sign_bad"):
        assert m[k].size == 0, (what, k, int(m[k].size), [describe(i) for i in m[k][:4]])
    yard = p64.YARDSTICK[P["name"]]
    ratio = {k: np.max(m[k] / np.maximum(np.array(yard[k]), 1e-300) * (np.array(yard[k]) > 0)) for k in ("t", "pt", "nrm")}
    return m, ratio


@pytest.mark.parametrize("arith", MODES)
@pytest.mark.parametrize("name", p64.SCENES)
def test_primitive_tests_per_ray(prepared, name, arith):
    P = prepared(name)
    P["name"] = name
    n = P["rays"]["o"].shape[1]
    order = np.random.default_rng(7).permutation(n)  # the small runs mix the families
    r = capi.Renderer(P["scene"], arith=arith)
    try:
        assert r.stats().tight_leaves == 0
        runs = [order[:k] for k in (1, 63, 64, 65)] + [np.arange(n)]
        for idx in runs:
            got = r.stage_intersect(np.ascontiguousarray(P["rays"]["o"][:, idx]), np.ascontiguousarray(P["rays"]["d"][:, idx]))
            what = f"{name} {arith} n={len(idx)}"
            m, ratio = check(arith, what, P, idx, got)
            yard = p64.YARDSTICK[name]
            if len(idx) == n:
                np.set_printoptions(linewidth=250, precision=2)
                print(f"PRIM {what}: clear rays {int(P['ref']['clear'].sum())}, max over geoms of error / yardstick: t {ratio['t']:.2f} pt {ratio['pt']:.2f} nrm {ratio['nrm']:.2f}"
                      f"\n  t   {m['t'] / np.array(yard['t'])}\n  pt  {m['pt'] / np.array(yard['pt'])}")
            for k in ("t", "pt", "nrm"):
                over = np.flatnonzero(m[k] > FACTOR * np.array(yard[k]))
                assert over.size == 0, (what, k, over.tolist(), (m[k][over] / np.array(yard[k])[over]).tolist())
    finally:
        r.free()
