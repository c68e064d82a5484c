"""The history across a moved object simulated on the CPU (no GPU): the oracle's samples through the library's host functions
(pt_history_motion_host, pt_history_reproject_motion_host with the moments kind, the captures and the blend), in the command line's
order.  Cornell 96 x 54 at depth 8 with the sphere made diffuse (material 2); the camera stands still and the sphere's TRANS x goes
from -2.5 in steps of 0.5 over 8 views, 4 spp per view over disjoint iteration ranges, the default options; scored against 1024 spp
(iterations 100001 ...) of the last view.  The same sequence with the plain lookup, which treats the world as static, beside it: the
figures README and DESIGN.md section 10 quote, and the numbers the exact build must reproduce on the device
(tests/test_gpu_history_motion.py)."""
import os

import numpy as np
import pytest

import features_ref
import history_motion_ref as ref
import history_ref as href


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    from oracle import binding as ob
    paths = ref.sim_scene_paths(tmp_path_factory.mktemp("history_motion_sim"))
    threads = min(os.cpu_count() or 1, 16)
    ob.set_math_mode(ob.PORTABLE)
    try:
        views = []
        for f, path in enumerate(paths):
            feat = href.pack_features(features_ref.iteration_values(ob, path, href.RES, False, 1))
            ob.load_scene(path, res=href.RES)
            assert ob.trace_depth() == 8
            sc = capi.Scene(path, res=href.RES)
            views.append((sc.camera, ref.copy_geoms(sc), ob.render(f * href.SPP + 1, href.SPP, variant=ob.RETIRE, nthreads=threads), feat))
        truth = ob.render(href.TRUTH_FIRST, href.TRUTH_SPP, variant=ob.RETIRE, nthreads=threads).astype(np.float64) / href.TRUTH_SPP
    finally:
        ob.set_math_mode(ob.LIBM)
    reject = capi.reject_geoms(capi.Scene(paths[0], res=href.RES))
    assert not reject[ref.SPHERE]  # diffuse: its pixels may carry history
    return dict(views=views, truth=truth, reject=reject)


def test_the_motion_lookup_follows_the_sphere(sim):
    w, h = href.RES
    fns = ref.host_functions(sim["reject"], w, h)
    _, _, S, feat = sim["views"][-1]
    moving = ref.sphere_scores(ref.run_sequence(sim["views"], fns), feat, S, sim["truth"])
    static = ref.sphere_scores(ref.run_sequence(sim["views"], fns, motion=False), feat, S, sim["truth"])
    print(f"sphere step {ref.SPHERE_STEP}, last view: {moving['pixels']} sphere pixels, carried {static['carried']} plain / {moving['carried']} motion "
          f"(mean Th {static['weight']:.3g} / {moving['weight']:.3g}); MSE over the sphere raw {moving['raw']:.9g}, plain {static['sphere']:.9g}, "
          f"motion {moving['sphere']:.9g}; over the frame plain {static['frame']:.9g}, motion {moving['frame']:.9g}")
    assert moving["pixels"] == static["pixels"] > 20
    assert moving["carried"] > static["carried"]
    assert moving["sphere"] < static["sphere"]
    assert moving["sphere"] < moving["raw"]
    assert moving["frame"] <= static["frame"]
    assert (moving["pixels"], static["carried"], moving["carried"]) == (ref.SIM_SPHERE_PIXELS, ref.SIM_CARRIED_PLAIN, ref.SIM_CARRIED_MOTION)
    for got, pinned in ((moving["raw"], ref.SIM_SPHERE_RAW), (static["sphere"], ref.SIM_SPHERE_PLAIN), (moving["sphere"], ref.SIM_SPHERE_MOTION),
                        (static["frame"], ref.SIM_FRAME_PLAIN), (moving["frame"], ref.SIM_FRAME_MOTION)):
        assert abs(got / pinned - 1) < 1e-6, (got, pinned)


def test_the_restatement_runs_the_same_sequence(sim):
    """tests/history_motion_ref.py in the host functions' place: the same blends and planes, bit for bit."""
    w, h = href.RES
    want = ref.run_sequence(sim["views"], ref.host_functions(sim["reject"], w, h))
    got = ref.run_sequence(sim["views"], ref.ref_functions(sim["reject"], w, h))
    moved_pixels = 0
    for f, (a, b) in enumerate(zip(got, want)):
        for x, y in zip(a, b):
            assert (x is None) == (y is None), f
            if x is not None:
                assert np.array_equal(ref.bits(x), ref.bits(y)), f
    for f in range(1, len(want)):
        _, kind = ref.motion_table(sim["views"][f - 1][1], sim["views"][f][1])
        assert list(kind) == [ref.STILL] * ref.SPHERE + [ref.MOVED]
        moved_pixels += int((want[f][1][:, 3] > 0).sum())
    assert moved_pixels > 0
