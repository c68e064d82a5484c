"""The history probes under material edits (pt_history_probe_keep / _check after pt_set_materials): the replay property — nothing
edited, nothing changed —, a dimmed light seen by the probes of every surface it lights while its own probes are skipped, and the
device's L against pt_history_probe_gradient_host on the read-back inputs, in all three arithmetic modes."""
import numpy as np
import pytest

import history_materials_ref as mref
import history_motion_ref as mot
import history_ref as href
from history_ref import bits, f32

pytestmark = pytest.mark.gpu
RES = href.RES
W, H = RES
SPP = href.SPP
MOM, MATERIALS = mref.MOMENTS, mref.MATERIALS
LIGHT, LIGHT_GEOM, PHASE = 0, 0, 4


def same(got, want, what=""):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


@pytest.fixture(scope="module")
def scene_path(tmp_path_factory):
    return mot.sim_scene_paths(tmp_path_factory.mktemp("gpu_history_probe_materials"), frames=1)[0]  # cornell 96 x 54, depth 8, the sphere diffuse


def dim(scene, r, emittance):
    m = scene.material(LIGHT)
    m.emittance = float(f32(emittance))
    scene.set_material(LIGHT, m)
    r.set_materials(scene)


def looked_up_view(r, first):
    r.render(first, SPP)
    r.render_features(1, 1)
    r.history_reproject_ex(MOM | MATERIALS)


@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
def test_probes_see_a_dimmed_light_and_nothing_else(scene_path, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(scene_path, res=RES)
    lst = capi.history_probe_list_host(W, H, PHASE)
    P = lst.size
    r = capi.Renderer(scene, arith=arith)
    try:
        r.render(1, SPP)
        r.render_features(1, 1)
        r.history_probe_keep(1, SPP, PHASE)
        r.history_capture_ex(SPP, MOM)
        PK = r.readback_history_probe()[0]
        ids = href.surface(r.readback_feature_planes())[3]
        misses, lit = int((ids[lst] == 0).sum()), int((ids[lst] == LIGHT_GEOM + 1).sum())
        assert lit > 0

        def unchanged(what):
            C0 = r.readback_history()[1]
            assert (C0[:, 3] > 0).any()
            assert r.history_probe_check(radius=4, gain=8.0) == (P, 0, misses), what
            same(r.readback_history()[1], C0, what)
            L = r.readback_history_probe()[1]
            assert int((bits(L) == 0).sum()) == P - misses and int((L == -1).sum()) == misses, what

        # the same materials again: nothing changed
        r.set_materials(scene)
        looked_up_view(r, 101)
        unchanged("after pt_set_materials with the same materials")
        # an edit and the edit back
        dim(scene, r, 0.75)
        dim(scene, r, 1.5)
        looked_up_view(r, 201)
        unchanged("after an edit and the edit back")
        # the light dimmed
        dim(scene, r, 0.75)
        looked_up_view(r, 301)
        feat, C0 = r.readback_feature_planes(), r.readback_history()[1]
        VC0 = r.readback_history_variance()[1]
        assert not C0[ids == LIGHT_GEOM + 1].any()  # the lookup dropped the light's own history
        probes, changed, skipped = r.history_probe_check(gain=1.0)
        C1 = r.readback_history()[1]
        PK1, L = r.readback_history_probe()
        same(PK1, PK, "PK after pt_set_materials and pt_clear")
        assert (probes, skipped) == (P, misses + lit) and changed > 0  # the light's own probes are among the skipped
        assert (L[ids[lst] == LIGHT_GEOM + 1] == -1).all()
        same(C1[:, :3], C0[:, :3], "only C.w differs"), same(r.readback_history_variance()[1], VC0, "VC")
        assert (C1[:, 3] < C0[:, 3]).any() and not (C1[:, 3] > C0[:, 3]).any()
        # a sample that ended on the light gave half of what it gave; one that left the box for the sky or ran out of depth gave what it
        # gave: L is between 0 and 0.5 wherever the kept sum was not zero, and exactly zero where it was
        replayed = L >= 0
        lit_probes = replayed & (PK[:, :3].sum(axis=1) > 0)
        print(f"[{arith}] {P} probes: changed {changed}, skipped {skipped}; with a kept sum {int(lit_probes.sum())}, of those L: "
              f"{np.unique(np.round(L[lit_probes], 4), return_counts=True)}")
        assert lit_probes.sum() > 100 and (L[lit_probes] <= 0.5 + 1e-6).all() and int((L > 0).sum()) == changed
        assert (bits(L[replayed & ~lit_probes]) == 0).all()
        # ... and the device's L is the host's on the read-back inputs
        Sw = capi.stage_render_list_capacity(lst, P, 1, SPP)  # the kept iterations of the probes' pixels in the world as it is now
        moved = np.zeros(scene.desc.num_geoms, np.uint8)
        moved[LIGHT_GEOM] = 1
        want_L, want_changed, want_skipped = capi.history_probe_gradient_host(PK, Sw, feat, W, H, PHASE, moved)
        same(L, want_L, "L")
        assert (changed, skipped) == (want_changed, want_skipped)
        same(C1, capi.history_probe_apply_host(C0, want_L, feat, W, H, PHASE, moved, gain=1.0), "C")
    finally:
        r.free()
