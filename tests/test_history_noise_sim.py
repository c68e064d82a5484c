"""Rendering a view until the blend is clean, simulated on the CPU (no GPU): the oracle's samples through the library's host functions
(pt_noise_fold_host, pt_history_noise_host, pt_history_capture_host / _capture_variance_host / _reproject_variance_host / _blend_host).
The orbit of tests/test_history_sim.py — cornell 96 x 54, depth 8, 8 views 3 degrees apart — with view f rendering iterations
16 f + 1 ... in groups of 1, a fold after each, at most 16 of them, under two rules: pt_render_until's (the view's own estimate) and
pt_history_render_until's (the estimate of the blend with the carried history).  The truth is 1024 spp (iterations 100001 ...) at
each view's own camera.  The figures are those README "Noise estimate of the blend" quotes and the exact build reproduces on the
device (tests/test_gpu_history_noise.py).  The calibration of the estimate (estimated over actual squared error of the blend) is
recorded, not bounded."""
import os

import numpy as np
import pytest

import features_ref
import history_noise_ref as ref
import history_ref as href
import noise_ref


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    from oracle import binding as ob
    paths = href.orbit_scene_paths(tmp_path_factory.mktemp("history_noise_sim"))
    threads = min(os.cpu_count() or 1, 16)
    n = href.RES[0] * href.RES[1]
    ob.set_math_mode(ob.PORTABLE)
    try:
        views, truths = [], []
        for f, path in enumerate(paths):
            feat = href.pack_features(features_ref.iteration_values(ob, path, href.RES, False, 1))
            ob.load_scene(path, res=href.RES)
            assert ob.trace_depth() == 8
            S, noise = None, noise_ref.new_planes(n)
            sums, planes, sses = [], [], []
            for t in range(1, ref.CAP + 1):
                S = ob.render(f * ref.CAP + t, ref.GROUP, variant=ob.RETIRE, nthreads=threads, accum=S)
                sses.append(capi.noise_fold_host(S, noise, ref.GROUP, t, t))
                sums.append(S.copy()), planes.append(noise.copy())
            views.append((capi.Scene(path, res=href.RES).camera, feat, sums, planes, sses))
            truths.append(ob.render(href.TRUTH_FIRST, href.TRUTH_SPP, variant=ob.RETIRE, nthreads=threads).astype(np.float64) / href.TRUTH_SPP)
    finally:
        ob.set_math_mode(ob.LIBM)
    reject = capi.reject_geoms(capi.Scene(paths[0], res=href.RES))
    w, h = href.RES
    return {target: ref.run_rules(views, truths, reject, w, h, target) for target in ref.TARGETS}


@pytest.mark.parametrize("target", ref.TARGETS)
def test_the_blends_rule_against_the_views_own(sim, target):
    rows = sim[target]
    for f, r in enumerate(rows):
        print(f"target {target} dB, view {f}: alone {r['alone']} iterations ({r['alone_db']:.4f} dB), blend {r['blend']} iterations, estimated "
              f"{r['est_db']:.4f} dB, actual {r['actual_db']:.4f} dB, estimated / actual squared error {r['ratio']:.4f}, the view alone there "
              f"{r['view_db_at_stop']:.4f} dB; closest estimate to the target {min(abs(p - target) for p in r['looked']):.5f} dB")
    # the digits of the first run
    assert tuple(r["alone"] for r in rows) == ref.SIM_ALONE[target]
    assert tuple(r["blend"] for r in rows) == ref.SIM_BLEND[target]
    for r, est, actual, ratio in zip(rows, ref.SIM_EST_DB[target], ref.SIM_ACTUAL_DB[target], ref.SIM_RATIO[target]):
        assert abs(r["est_db"] - est) < 5e-4 and abs(r["actual_db"] - actual) < 5e-4 and abs(r["ratio"] - ratio) < 5e-4, (r, est, actual, ratio)
    # view 0 has no history: the two rules are one
    assert rows[0]["alone"] == rows[0]["blend"] and rows[0]["est_db"] == rows[0]["view_db_at_stop"]
    # from view 1 on the blend's rule takes no more iterations than the view's own
    assert all(r["blend"] <= r["alone"] for r in rows[1:])
    assert sum(r["blend"] for r in rows[1:]) < sum(r["alone"] for r in rows[1:])
    # no decision of either rule lies within the margin of the target: the last bits of the device's double cannot flip one
    assert min(abs(p - target) for r in rows for p in r["looked"]) >= ref.MARGIN_DB


def test_the_view_alone_stops_below_the_cap_at_one_target(sim):
    assert any(all(r["alone"] < ref.CAP for r in sim[target][1:]) for target in ref.TARGETS)
