"""The filter over the blend simulated on the CPU (no GPU): the oracle's samples through the library's host functions
(pt_noise_fold_host, pt_history_capture_host / _capture_variance_host / _reproject_variance_host / _blend_host / _denoise_host), in the
command line's --denoise-history order.  The orbit of tests/test_history_sim.py — cornell 96 x 54, depth 8, 8 views 3 degrees apart,
4 spp per view over disjoint iteration ranges — with the 4 spp of a view in 4 groups of 1 and a fold after each, default options,
scored against 1024 spp (iterations 100001 ...) at the last camera.  History plus filter must beat either alone: the filtered blend
against (a) the unfiltered blend, history_ref.SIM_CARRIED, and (b) pt_denoise_guided_host on the last view's own 4 spp without history.
The figures are those README "Variance of the history" quotes and the exact build reproduces on the device
(tests/test_gpu_history_variance.py).  The calibration of the carried variance (its sum against the blend's actual squared error) is
recorded, not bounded: the estimate is biased by the lookup, which interpolates the variance as if the taps were one sample."""
import os

import numpy as np
import pytest

import features_ref
import history_ref as href
import history_variance_ref as ref
import noise_ref


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    from oracle import binding as ob
    paths = href.orbit_scene_paths(tmp_path_factory.mktemp("history_variance_sim"))
    threads = min(os.cpu_count() or 1, 16)
    n = href.RES[0] * href.RES[1]
    per_group = href.SPP // ref.GROUPS
    ob.set_math_mode(ob.PORTABLE)
    try:
        views = []
        for f, path in enumerate(paths):
            feat = href.pack_features(features_ref.iteration_values(ob, path, href.RES, False, 1))
            ob.load_scene(path, res=href.RES)
            assert ob.trace_depth() == 8
            S, noise, T = None, noise_ref.new_planes(n), 0
            for M in range(1, ref.GROUPS + 1):
                S = ob.render(f * href.SPP + T + 1, per_group, variant=ob.RETIRE, nthreads=threads, accum=S)
                T += per_group
                capi.noise_fold_host(S, noise, per_group, M, T)
            views.append((capi.Scene(path, res=href.RES).camera, S, feat, noise))
        truth = ob.render(href.TRUTH_FIRST, href.TRUTH_SPP, variant=ob.RETIRE, nthreads=threads).astype(np.float64) / href.TRUTH_SPP
    finally:
        ob.set_math_mode(ob.LIBM)
    reject = capi.reject_geoms(capi.Scene(paths[0], res=href.RES))
    return dict(views=views, truth=truth, reject=reject)


def test_history_plus_filter_beats_either_alone(sim):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, h = href.RES
    out = ref.run_orbit(sim["views"], ref.host_functions(sim["reject"], w, h))
    truth = sim["truth"]
    blend, filtered, C, VC, K, VK = out[-1]
    _, S, feat, noise = sim["views"][-1]
    carried = href.mse(blend, truth)
    both = href.mse(filtered, truth)
    alone = href.mse(capi.denoise_guided_host(S, feat, noise, w, h, ref.GROUPS, href.SPP), truth)
    sum_var, sum_err2 = ref.calibration(VK, blend, truth)
    print(f"orbit, last view: MSE blend {carried:.6g}, filtered blend {both:.6g} ({both / carried:.4f} of the blend), guided filter on the view's own "
          f"{href.SPP} spp {alone:.6g} ({both / alone:.4f} of it); sum of the carried variance {sum_var:.6g} against the blend's squared error "
          f"{sum_err2:.6g} (ratio {sum_var / sum_err2:.4f})")
    assert abs(carried - href.SIM_CARRIED) < 1e-7  # the blend is the plain history's: the variance side changes no colour
    assert both < carried    # (a)
    assert both < alone      # (b)
    assert abs(both - ref.SIM_FILTERED) < 1e-7 and abs(alone - ref.SIM_GUIDED_ALONE) < 1e-7
    assert abs(sum_var / ref.SIM_SUM_VAR - 1) < 1e-7 and abs(sum_err2 / ref.SIM_SUM_ERR2 - 1) < 1e-7  # (sums of ~10: relative)
    assert abs(both / carried - ref.SIM_FILTERED_OF_CARRIED) < 1e-4 and abs(both / alone - ref.SIM_FILTERED_OF_GUIDED) < 1e-4


def test_the_restatement_runs_the_same_orbit(sim):
    """tests/history_variance_ref.py in the host functions' place: the same planes and images, bit for bit, over three views."""
    w, h = href.RES
    views = sim["views"][:3]
    want = ref.run_orbit(views, ref.host_functions(sim["reject"], w, h))
    got = ref.run_orbit(views, ref.ref_functions(sim["reject"], w, h))
    names = ("blend", "filtered", "C", "VC", "K", "VK")
    for f, (a, b) in enumerate(zip(got, want)):
        for name, x, y in zip(names, a, b):
            if x is None or y is None:
                assert x is None and y is None, (f, name)
            else:
                assert np.array_equal(href.bits(x), href.bits(y)), (f, name)
    assert (want[2][3][:, :3] > 0).any()  # a variance was carried
