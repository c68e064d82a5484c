"""The simulations of tests/test_history_materials_sim.py on one renderer: the exact build reproduces the oracle's samples bit for bit, so
pt_set_materials before view 4, render, features, the lookup (with and without PT_HISTORY_MATERIALS), the probes' check and keep, resolve
and capture over the 8 views give the same digits."""
import numpy as np
import pytest

import history_materials_ref as ref
import history_ref as href

pytestmark = pytest.mark.gpu
SPP = href.SPP


def run(r, capi, after, flagged=True, probes=None):
    """One sequence from the renderer's first scene; returns (the last view's blend, C, S, feature planes, (changed, skipped) per view)."""
    counts = []
    for f in range(href.FRAMES):
        if f == ref.EDIT_VIEW:
            r.set_materials(after)
        else:
            r.clear()
        r.render(f * SPP + 1, SPP)
        r.render_features(1, 1)
        if f > 0:
            r.history_reproject_ex(ref.MOMENTS | (ref.MATERIALS if flagged else 0))
            if probes is not None:
                counts.append(r.history_probe_check(radius=probes[0] or -1, gain=probes[1])[1:])
        if probes is not None:
            r.history_probe_keep(f * SPP + 1, SPP, f % 9)
        blend = r.history_resolve(SPP)
        r.history_capture_ex(SPP, ref.MOMENTS)
    return blend, r.readback_history()[1], r.readback(), r.readback_feature_planes(), counts


def truth_of(r):
    r.clear()
    r.render(href.TRUTH_FIRST, href.TRUTH_SPP)
    return r.readback().astype(np.float64) / href.TRUTH_SPP


def close(got, pinned):
    return got == pinned if isinstance(pinned, int) else abs(got / pinned - 1) < 1e-6


def test_the_recolour_sequence_on_the_device(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    before, after = (capi.Scene(p, res=href.RES) for p in ref.sim_scene_paths(tmp_path, "recolour"))
    out = {}
    for flagged in (True, False):
        r = capi.Renderer(before, arith="exact")
        try:
            out[flagged] = run(r, capi, after, flagged)
            truth = truth_of(r)
        finally:
            r.free()
    blend, C, S, feat, _ = out[True]
    hit, _, _, ids = href.surface(feat)
    wall = hit & (ids == ref.SIM_WALL_GEOM + 1)
    raw = np.asarray(S, np.float64) / SPP
    got = dict(pixels=int(wall.sum()), carried=int((C[wall, 3] > 0).sum()), wall_raw=href.mse(raw[wall], truth[wall]),
               wall_plain=href.mse(out[False][0][wall], truth[wall]), wall_flagged=href.mse(blend[wall], truth[wall]), rest_raw=href.mse(raw[~wall], truth[~wall]),
               rest_plain=href.mse(out[False][0][~wall], truth[~wall]), rest_flagged=href.mse(blend[~wall], truth[~wall]))
    print("on the device, recolour, last view: " + ", ".join(f"{k} {v:.9g}" if isinstance(v, float) else f"{k} {v}" for k, v in got.items()))
    assert got["wall_flagged"] < got["wall_plain"]
    for k, pinned in ref.SIM_RECOLOUR.items():
        assert close(got[k], pinned), (k, got[k], pinned)


def test_the_dimmed_light_sequence_on_the_device(tmp_path):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    before, after = (capi.Scene(p, res=href.RES) for p in ref.sim_scene_paths(tmp_path, "dimmed"))
    got, counts, truth = {}, None, None
    for name, probes in [("none", None)] + [(f"r{radius}g{gain:g}", (radius, gain)) for radius, gain in ref.PROBE_SCAN]:
        r = capi.Renderer(before, arith="exact")
        try:
            blend, _, _, _, c = run(r, capi, after, True, probes)
            if truth is None:
                truth = truth_of(r)
        finally:
            r.free()
        got[name] = href.mse(blend, truth)
        if probes is not None and counts is None:
            counts = c
    print("on the device, dimmed light, frame MSE at the last view: " + ", ".join(f"{k} {v:.9g}" for k, v in got.items()) + f"; (changed, skipped) per view {counts}")
    assert min(v for k, v in got.items() if k != "none") < got["none"]
    assert [tuple(c) for c in counts] == ref.SIM_DIMMED_COUNTS
    for k, pinned in ref.SIM_DIMMED.items():
        assert close(got[k], pinned), (k, got[k], pinned)
