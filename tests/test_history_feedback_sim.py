"""The feedback simulated on the CPU (no GPU): the oracle's samples through the library's host functions, in the command line's
--denoise-history --history-moments --history-feedback order (lookup, round, filter, capture).  The orbit of
tests/test_history_moments_sim.py — cornell 96 x 54, depth 8, 8 views 3 degrees apart, 1 spp per view, view f rendering iteration
f + 1 — scored against 1024 spp at the last camera, for the tap after level L = 1 .. 5 and both variance rules, in three cases: without
rounds (without feedback: history_moments_ref.SIM_FILTERED), with rounds of 3 (tests/test_history_round_sim.py's samples; without
feedback: history_round_ref.SIM_ROUND_FILTERED), and with the camera standing still at the last camera, where the mean squared
difference between the filtered outputs of views 7 and 8 — flicker — is taken too.  No figure was fixed in advance: the test prints what
it measures and pins it as a recorded result; README "Feedback" quotes the table, and the exact build reproduces the defaults' digits
on the device (tests/test_gpu_history_feedback.py).  One scene, one orbit: no claim beyond it."""
import os

import numpy as np
import pytest

import features_ref
import history_feedback_ref as ref
import history_moments_ref as mref
import history_ref as href
import history_round_ref as rref

LEVELS = (1, 2, 3, 4, 5)
RULES = (0, 1)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    from oracle import binding as ob
    paths = href.orbit_scene_paths(tmp_path_factory.mktemp("history_feedback_sim"))
    threads = min(os.cpu_count() or 1, 16)
    G = rref.SIM_GROUP
    ob.set_math_mode(ob.PORTABLE)
    try:
        views, groups = [], []
        for f, path in enumerate(paths):
            feat = href.pack_features(features_ref.iteration_values(ob, path, href.RES, False, 1))
            ob.load_scene(path, res=href.RES)
            assert ob.trace_depth() == 8
            cam = capi.Scene(path, res=href.RES).camera
            views.append((cam, ob.render(f + 1, 1, variant=ob.RETIRE, nthreads=threads), feat))
            groups.append(ob.render(1000 + f * G + 1, G, variant=ob.RETIRE, nthreads=threads))  # the round's samples, every pixel's
        # the camera standing still at the last camera (the scene is loaded): view f renders iteration f + 1 there
        still = [(views[-1][0], ob.render(f + 1, 1, variant=ob.RETIRE, nthreads=threads), views[-1][2]) for f in range(len(paths))]
        truth = ob.render(href.TRUTH_FIRST, href.TRUTH_SPP, variant=ob.RETIRE, nthreads=threads).astype(np.float64) / href.TRUTH_SPP
    finally:
        ob.set_math_mode(ob.LIBM)
    scene = capi.Scene(paths[0], res=href.RES)
    return dict(views=views, groups=groups, still=still, truth=truth, reject=capi.reject_geoms(scene), emitter=capi.emitter_geoms(scene))


def round_fn(sim):
    """The history round of tests/test_history_round_sim.py between the lookup and the filter: its lists follow from the raw chain alone."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, h = href.RES

    def go(f, S, feat, C):
        E = np.zeros(w * h, np.float32)
        lst, _, m = capi.history_select_host(feat, w, h, C, sim["emitter"], 0.0, 0.0)
        if m:
            S, E = capi.history_merge_host(S, E, lst[:m], sim["groups"][f][np.asarray(lst[:m])], rref.SIM_GROUP)
        return S, E
    return go


def flicker(out):
    a, b = (np.asarray(out[k][0], np.float64) for k in (-2, -1))
    return float(((a - b) ** 2).mean())


def table(rows):
    return "\n".join(f"  L = {L}:  rule 0  {r[0]:.9g}   rule 1  {r[1]:.9g}" for L, r in zip(LEVELS, rows))


def test_what_the_feedback_buys(sim):
    w, h = href.RES
    truth = sim["truth"]
    fns = ref.host_functions(sim["reject"], w, h)
    orbit, rounds, still, flick = [], [], [], []
    for L in LEVELS:
        o, r, s, k = [], [], [], []
        for V in RULES:
            o.append(href.mse(ref.run_orbit(sim["views"], fns, 1, L, V)[-1][0], truth))
            r.append(href.mse(ref.run_orbit(sim["views"], fns, 1, L, V, round_fn(sim))[-1][0], truth))
            out = ref.run_orbit(sim["still"], fns, 1, L, V)
            s.append(href.mse(out[-1][0], truth)), k.append(flicker(out))
        orbit.append(o), rounds.append(r), still.append(s), flick.append(k)
    # without feedback: the moments filter on the same three sequences
    base = mref.run_orbit(sim["views"], mref.host_functions(sim["reject"], w, h), 1)
    base_rounds = rref.run_orbit(sim["views"], rref.host_functions(sim["reject"], w, h), 1, rref.SIM_GROUP,
                                 lambda f, lst: sim["groups"][f][np.asarray(lst)], emitter=sim["emitter"])
    base_still = mref.run_orbit(sim["still"], mref.host_functions(sim["reject"], w, h), 1)
    still_flick = float(((np.asarray(base_still[-2][1], np.float64) - np.asarray(base_still[-1][1], np.float64)) ** 2).mean())
    without = [href.mse(base[-1][1], truth), href.mse(base_rounds[-1][1], truth), href.mse(base_still[-1][1], truth), still_flick]
    print("MSE of the filtered image at the last view, tap after level L, variance rule 0 / 1")
    print(f"the orbit, without rounds (without feedback {without[0]:.9g}):\n{table(orbit)}")
    print(f"the orbit, rounds of {rref.SIM_GROUP} (without feedback {without[1]:.9g}):\n{table(rounds)}")
    print(f"the camera standing still (without feedback {without[2]:.9g}):\n{table(still)}")
    print(f"... and its flicker, the mean squared difference of views 7 and 8 (without feedback {without[3]:.9g}):\n{table(flick)}")
    fmt = lambda rows: "[" + ", ".join("[" + ", ".join(f"{x:.9g}" for x in r) + "]" for r in rows) + "]"  # noqa: E731
    print(f"recorded: SIM_ORBIT = {fmt(orbit)}\nSIM_ROUNDS = {fmt(rounds)}\nSIM_STILL = {fmt(still)}\nSIM_FLICKER = {fmt(flick)}\nSIM_WITHOUT = {fmt([without])[1:-1]}")
    assert abs(without[0] / mref.SIM_FILTERED - 1) < 1e-6 and abs(without[1] / rref.SIM_ROUND_FILTERED - 1) < 1e-6  # the parent's figures
    for got, pinned in ((orbit, ref.SIM_ORBIT), (rounds, ref.SIM_ROUNDS), (still, ref.SIM_STILL), (flick, ref.SIM_FLICKER), ([without], [ref.SIM_WITHOUT])):
        assert pinned is not None, "nothing recorded yet"
        assert np.allclose(np.asarray(got), np.asarray(pinned), rtol=1e-6, atol=0), (got, pinned)
    # the defaults would be level 1, rule 0 unless another pair is lower on both the orbit and the still camera: the rule-1 pairs are,
    # (1, 1) most of all, and that is what PtHistoryFeedbackOptions' zeros mean
    better = [(L, V) for i, L in enumerate(LEVELS) for V in RULES if orbit[i][V] < orbit[0][0] and still[i][V] < still[0][0]]
    assert better == ref.SIM_BETTER_THAN_DEFAULTS, better
    L0, V0 = ref.DEFAULTS
    assert all(orbit[L0 - 1][V0] <= orbit[L - 1][V] and still[L0 - 1][V0] <= still[L - 1][V] for L, V in better)
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    out = ref.run_orbit(sim["views"][:3], fns, 1, 0, None)  # the library's own defaults
    want = ref.run_orbit(sim["views"][:3], fns, 1, L0, V0)
    assert np.array_equal(href.bits(out[-1][0]), href.bits(want[-1][0])) and capi.HISTORY_FEEDBACK == ref.FEEDBACK
    # what the figures say, recorded as they fell: on this scene and orbit feedback LOSES to the filter without it in every case and
    # under every pair, in error and in flicker alike
    assert min(min(r) for r in orbit) > without[0] and min(min(r) for r in rounds) > without[1] and min(min(r) for r in still) > without[2]
    assert min(min(r) for r in flick) > without[3]


def test_the_raw_chain_is_the_moments_orbit(sim):
    """K, VK, C and VC of the orbit with feedback are those of the orbit without, bit for bit, and so are the rounds' extra planes."""
    w, h = href.RES
    views = sim["views"][:3]
    fns = ref.host_functions(sim["reject"], w, h)
    got = ref.run_orbit(views, fns, 1, 2, 1, round_fn(sim))
    base = rref.run_orbit(views, rref.host_functions(sim["reject"], w, h), 1, rref.SIM_GROUP, lambda f, lst: sim["groups"][f][np.asarray(lst)],
                          emitter=sim["emitter"])
    for f in range(3):
        assert np.array_equal(href.bits(got[f][7]), href.bits(base[f][5])), (f, "E")
    plain = mref.run_orbit(views, mref.host_functions(sim["reject"], w, h), 1)
    got = ref.run_orbit(views, fns, 1, 2, 1)
    for f in range(3):
        for name, a, b in (("C", got[f][1], plain[f][2]), ("VC", got[f][2], plain[f][3]), ("K", got[f][4], plain[f][4]), ("VK", got[f][5], plain[f][5])):
            if a is None:
                assert b is None
            else:
                assert np.array_equal(href.bits(a), href.bits(b)), (f, name)
