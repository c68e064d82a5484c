"""The history round simulated on the CPU (no GPU): the oracle's samples through the library's host functions (pt_history_select_host /
_merge_host and the counted twins of blend, capture, moments and filter), in the command line's --denoise-history --history-moments
--history-extra order.  The orbit of tests/test_history_moments_sim.py — cornell 96 x 54, depth 8, 8 views 3 degrees apart, 1 spp per
view, view f rendering iteration f + 1 — so the baseline is exactly history_moments_ref's pinned SIM_BLEND and SIM_FILTERED.  The
round's samples are the oracle's iterations 1000 + f G + 1 .. of view f, taken at the listed pixels (the oracle's samples are keyed by
iteration and pixel; the numbers are disjoint from the views' and from the truth's).  Scored against the same 1024 spp at the last
camera.  G = 3 with the default min_history = 4: one round brings a pixel that carries nothing to 1 + 3 = 4 samples, so it is not
selected again.  The figures are those README "History-guided sampling" quotes and the exact build reproduces on the device
(tests/test_gpu_history_round.py)."""
import os

import numpy as np
import pytest

import features_ref
import history_moments_ref as mref
import history_ref as href
import history_round_ref as ref


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    from oracle import binding as ob
    paths = href.orbit_scene_paths(tmp_path_factory.mktemp("history_round_sim"))
    threads = min(os.cpu_count() or 1, 16)
    G = ref.SIM_GROUP
    ob.set_math_mode(ob.PORTABLE)
    try:
        views, views2, groups = [], [], []
        for f, path in enumerate(paths):
            feat = href.pack_features(features_ref.iteration_values(ob, path, href.RES, False, 1))
            ob.load_scene(path, res=href.RES)
            assert ob.trace_depth() == 8
            cam = capi.Scene(path, res=href.RES).camera
            views.append((cam, ob.render(f + 1, 1, variant=ob.RETIRE, nthreads=threads), feat))
            views2.append((cam, ob.render(2 * f + 1, 2, variant=ob.RETIRE, nthreads=threads), feat))  # for context: 2 uniform spp per view
            groups.append(ob.render(1000 + f * G + 1, G, variant=ob.RETIRE, nthreads=threads))       # the round's samples, every pixel's
        truth = ob.render(href.TRUTH_FIRST, href.TRUTH_SPP, variant=ob.RETIRE, nthreads=threads).astype(np.float64) / href.TRUTH_SPP
    finally:
        ob.set_math_mode(ob.LIBM)
    scene = capi.Scene(paths[0], res=href.RES)
    return dict(views=views, views2=views2, groups=groups, truth=truth, reject=capi.reject_geoms(scene), emitter=capi.emitter_geoms(scene))


def run(sim, fns, views=None):
    views = sim["views"] if views is None else views
    return ref.run_orbit(views, fns, 1, ref.SIM_GROUP, lambda f, lst: sim["groups"][f][np.asarray(lst)], emitter=sim["emitter"])


def test_extra_samples_for_short_histories(sim):
    w, h = href.RES
    n, truth, G = w * h, sim["truth"], ref.SIM_GROUP
    out = run(sim, ref.host_functions(sim["reject"], w, h))
    m = [len(o[2]) for o in out]
    fresh = [o[3] for o in out]
    hits = [int((np.asarray(feat, np.float32).reshape(3, -1, 4)[1, :, 3] > 0).sum()) for _, _, feat in sim["views"]]
    blend, filtered = href.mse(out[-1][0], truth), href.mse(out[-1][1], truth)
    samples = (len(out) * n + G * sum(m)) / (len(out) * n)
    two = mref.run_orbit(sim["views2"], mref.host_functions(sim["reject"], w, h), 2)
    blend2, filtered2 = href.mse(two[-1][0], truth), href.mse(two[-1][1], truth)
    print(f"orbit at 1 spp with rounds of {G} below {float(ref.MIN_HISTORY):g} samples, last view: MSE blend {blend:.9g} ({blend / mref.SIM_BLEND:.4f} of "
          f"{mref.SIM_BLEND:.9g} without), filtered blend {filtered:.9g} ({filtered / mref.SIM_FILTERED:.4f} of {mref.SIM_FILTERED:.9g} without); samples "
          f"{samples:.9g} x the baseline's; m per view {m}, fresh per view {fresh}, hit pixels per view {hits}; 2 uniform spp per view without rounds "
          f"(2 x the samples): blend {blend2:.9g}, filtered blend {filtered2:.9g}")
    for f in range(1, len(out)):  # from the second view on the selection is not trivial
        assert 0 < m[f] < hits[f], (f, m[f], hits[f])
    assert fresh == m  # no cap
    assert all(float(o[5].sum()) == G * len(o[2]) for o in out)
    assert samples <= 1.25
    assert blend < mref.SIM_BLEND
    assert filtered < mref.SIM_FILTERED
    assert m == ref.SIM_ROUND_M
    for got, pinned in ((blend, ref.SIM_ROUND_BLEND), (filtered, ref.SIM_ROUND_FILTERED), (samples, ref.SIM_ROUND_SAMPLES),
                        (blend2, ref.SIM_2SPP_BLEND), (filtered2, ref.SIM_2SPP_FILTERED)):
        assert abs(got / pinned - 1) < 1e-6, (got, pinned)


def test_without_fresh_pixels_it_is_the_baseline(sim):
    """Rounds that select nothing: E stays all zero, and the counted orbit's images are the uncounted orbit's of
    history_moments_ref, bit for bit, over three views."""
    w, h = href.RES
    views = sim["views"][:3]
    base = mref.run_orbit(views, mref.host_functions(sim["reject"], w, h), 1)
    fns = ref.host_functions(sim["reject"], w, h)
    fns["select"] = lambda feat, C, em, mh, mf: (np.zeros(0, np.int32), 0, 0)  # nothing fresh
    got = ref.run_orbit(views, fns, 1, ref.SIM_GROUP, None, emitter=sim["emitter"])
    for f in range(3):
        assert np.array_equal(href.bits(got[f][0]), href.bits(base[f][0])) and np.array_equal(href.bits(got[f][1]), href.bits(base[f][1])), f


def test_the_restatement_runs_the_same_orbit(sim):
    """tests/history_round_ref.py in the host functions' place: the same lists, images and extra planes, bit for bit, over three views."""
    w, h = href.RES
    views = sim["views"][:3]
    want = run(sim, ref.host_functions(sim["reject"], w, h), views)
    got = run(sim, ref.ref_functions(sim["reject"], w, h), views)
    for f, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a[2], b[2]) and a[3] == b[3], f
        for name, x, y in zip(("blend", "filtered", None, None, "S", "E"), a, b):
            if name:
                assert np.array_equal(href.bits(x), href.bits(y)), (f, name)
    assert 0 < len(want[1][2]) < len(want[0][2])
