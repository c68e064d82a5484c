"""Threshold rounds over the blend, simulated on the CPU (no GPU): the oracle's samples through the library's host functions
(pt_noise_fold_host, pt_adaptive_select_threshold_host / pt_history_select_threshold_blend_host, pt_adaptive_merge_host,
pt_history_*_adaptive_host, pt_history_reproject_variance_host).  The orbit of tests/test_history_noise_sim.py — cornell 96 x 54, depth
8, 8 views 3 degrees apart — with view f using the iteration numbers 16 f + 1 ... in groups of 2: two uniform groups with a fold after
each, then threshold rounds (max_fraction 1, until at most 5 pixels are above) at the same E under two rules: pt_render_threshold's
selection, every view on its own, and the blend's, with the history carried from view to view.  The truth is 1024 spp (iterations
100001 ...) at each view's own camera.  The figures are those README "Threshold rounds over the blend" quotes and the exact build
reproduces on the device (tests/test_gpu_history_threshold.py).  The calibration of the estimate is recorded, not bounded."""
import os

import numpy as np
import pytest

import features_ref
import history_ref as href
import history_threshold_ref as ref


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    from oracle import binding as ob
    paths = href.orbit_scene_paths(tmp_path_factory.mktemp("history_threshold_sim"))
    threads = min(os.cpu_count() or 1, 16)
    ob.set_math_mode(ob.PORTABLE)
    try:
        views, truths = [], []
        for f, path in enumerate(paths):
            feat = href.pack_features(features_ref.iteration_values(ob, path, href.RES, False, 1))
            u1, u2, groups = ref.oracle_view(ob, path, href.RES, f, threads)
            assert ob.trace_depth() == 8
            views.append((capi.Scene(path, res=href.RES).camera, feat, [u1, u2], groups))
            truths.append(ob.render(href.TRUTH_FIRST, href.TRUTH_SPP, variant=ob.RETIRE, nthreads=threads).astype(np.float64) / href.TRUTH_SPP)
    finally:
        ob.set_math_mode(ob.LIBM)
    reject = capi.reject_geoms(capi.Scene(paths[0], res=href.RES))
    w, h = href.RES
    return ref.run_orbit_rules(capi, views, truths, reject, w, h, ref.SIM_E)


def test_the_blends_rule_against_the_views_own(sim):
    for f, r in enumerate(sim):
        print(f"view {f}: alone {r['alone_used']} iteration numbers, {r['alone_rounds']} rounds, {r['alone_samples']} samples, {r['alone_above']} above; "
              f"blend {r['used']} iteration numbers, {r['rounds']} rounds, {r['samples']} samples, {r['above']} above; MSE of the blend {r['mse']:.6e}, "
              f"filtered {r['mse_filtered']:.6e}; {r['finished']} finished pixels, {r['finished_over']:.4f} of them off by more than E; "
              f"estimated / actual squared error {r['ratio']:.4f}")
    # the digits of the first run
    assert tuple(r["alone_used"] for r in sim) == ref.SIM_ALONE_USED and tuple(r["alone_samples"] for r in sim) == ref.SIM_ALONE_SAMPLES
    assert tuple(r["used"] for r in sim) == ref.SIM_BLEND_USED and tuple(r["samples"] for r in sim) == ref.SIM_BLEND_SAMPLES
    assert abs(sim[-1]["mse"] / ref.SIM_LAST_MSE - 1) < 1e-5 and abs(sim[-1]["mse_filtered"] / ref.SIM_LAST_MSE_FILTERED - 1) < 1e-5
    # view 0 has no history: the two rules are one
    assert (sim[0]["alone_used"], sim[0]["alone_samples"], sim[0]["alone_above"]) == (sim[0]["used"], sim[0]["samples"], sim[0]["above"])
    # over views 1 .. 7 the blend's rule takes fewer samples, in every view and in all
    assert all(r["samples"] < r["alone_samples"] for r in sim[1:])
    assert sum(r["samples"] for r in sim[1:]) < sum(r["alone_samples"] for r in sim[1:])
    # recorded, not bounded
    for r, over, ratio in zip(sim, ref.SIM_FINISHED_OVER, ref.SIM_RATIO):
        assert abs(r["finished_over"] - over) < 5e-4 and abs(r["ratio"] - ratio) < 5e-4, (r, over, ratio)


def test_the_view_alone_stops_below_the_cap(sim):
    assert any(r["alone_used"] < ref.ORBIT_CAP for r in sim[1:])
