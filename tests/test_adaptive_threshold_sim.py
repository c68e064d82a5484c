"""Adaptive sampling by threshold simulated on the CPU (no GPU): the oracle's samples through the numpy restatement of fold, key,
threshold selection and merge (tests/adaptive_threshold_ref.py simulate).  Cornell 96x54, depth 8, groups of 4, two uniform groups,
threshold 0.05, truth = 4096 spp of iterations 100001 ...: the figures DESIGN.md section 10 quotes, and the numbers the exact build
must reproduce on the device (tests/test_gpu_adaptive_threshold.py), where the same restatement runs on the renderer's own samples."""
import os

import numpy as np
import pytest

import adaptive_ref as ref
import adaptive_threshold_ref as tref

RES, G, THRESHOLD = (96, 54), 4, 0.05
N = RES[0] * RES[1]
# what the simulation gives, cap fraction 1.0
ROUNDS, SAMPLES, MAX_T, UNIFORM_GROUPS = 84, 200_160, 344, 86
FIRST_LENGTHS, LAST_LENGTHS = [2410, 2407, 2374], [3, 2, 2, 1]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    from cosc_4397_pathtracing_raytracing_project_amd import scenes
    from oracle import binding as ob
    path = scenes.write_scene(scenes.cornell_scene_text(), str(tmp_path_factory.mktemp("threshold_sim") / "cornell.txt"))
    threads = min(os.cpu_count() or 1, 16)
    cache = {}

    def group_sum(first, count, accum=None):
        """Iterations first .. first + count - 1 of every pixel, added in order to a copy of accum (None: to zero; those are kept:
        the runs below ask for the same groups)."""
        if accum is None and (first, count) in cache:
            return cache[(first, count)]
        out = ob.render(first, count, variant=ob.RETIRE, nthreads=threads, accum=None if accum is None else accum.copy())
        if accum is None:
            cache[(first, count)] = out
        return out

    ob.set_math_mode(ob.PORTABLE)
    try:
        ob.load_scene(path, res=RES)
        assert ob.trace_depth() == 8
        out = dict(full=tref.simulate(RES[0], RES[1], group_sum, G, THRESHOLD, 1.0, 400),
                   quarter=tref.simulate(RES[0], RES[1], group_sum, G, THRESHOLD, 0.25, 400),
                   min63=tref.simulate(RES[0], RES[1], group_sum, G, THRESHOLD, 1.0, 400, min_pixels=63))
        out["uniform_groups"], out["uniform_sums"] = tref.uniform_groups_to_criterion(RES[0], RES[1], group_sum, G, THRESHOLD, 120)
        out["truth"] = ob.render(100001, 4096, variant=ob.RETIRE, nthreads=threads).astype(np.float64) / 4096
    finally:
        ob.set_math_mode(ob.LIBM)
    return out


def mse(S, T, truth):
    return float(((np.asarray(S, np.float64) / T - truth) ** 2).mean())


def test_rounds_samples_and_list_lengths(sim):
    s = sim["full"]
    lengths = s["lengths"]
    assert (len(lengths), s["samples"], int(s["counts"][:, 0].max())) == (ROUNDS, SAMPLES, MAX_T)
    assert lengths[:3] == FIRST_LENGTHS and lengths[-4:] == LAST_LENGTHS and s["above"][-1] == 0 and s["above"][:-1] == lengths  # cap 1: every above-pixel
    assert s["samples"] == 2 * G * N + G * sum(lengths) == int(s["counts"][:, 0].astype(np.int64).sum())
    never = float(np.mean(s["counts"][:, 0] == 2 * G))
    short = [m for m in lengths if m < 64]
    print(f"threshold {THRESHOLD}: {len(lengths)} rounds, {s['samples']} samples = {s['samples'] / N:.1f} spp, max T {s['counts'][:, 0].max()}, never resampled "
          f"{never:.3f}, {len(short)} rounds under 64 pixels with {G * sum(short) / (G * sum(lengths)):.4f} of the adaptive samples")
    assert 0.51 < never < 0.53 and len(short) == 46 and 0.017 < sum(short) / sum(lengths) < 0.019


def test_mse_against_uniform_at_equal_samples_and_uniform_to_the_criterion(sim):
    s, truth = sim["full"], sim["truth"]
    adaptive = float(((ref.resolve(s["S"], s["counts"]).astype(np.float64) - truth) ** 2).mean())
    groups = s["samples"] // (G * N)  # uniform groups the adaptive samples pay for: 9 groups = 36 spp for 38.6
    uniform = mse(sim["uniform_sums"][groups - 1], groups * G, truth)
    err = np.sqrt(((ref.resolve(s["S"], s["counts"]).astype(np.float64) - truth) ** 2).sum(axis=1))
    print(f"MSE adaptive {adaptive:.4g}, uniform at {groups * G} spp {uniform:.4g}, ratio {adaptive / uniform:.4f}; uniform meets the criterion after "
          f"{sim['uniform_groups']} groups; pixels with an actual error above the threshold {np.mean(err > THRESHOLD):.3f}, above twice {np.mean(err > 2 * THRESHOLD):.4f}")
    assert groups == 9 and abs(adaptive - 3.809e-4) < 1e-7 and abs(uniform - 7.867e-4) < 1e-7 and abs(adaptive / uniform - 0.484) < 1e-3
    assert sim["uniform_groups"] == UNIFORM_GROUPS and abs(UNIFORM_GROUPS * G * N / s["samples"] - 8.9) < 0.05
    # the threshold is one sigma of an estimate, not a bound
    assert 0.13 < np.mean(err > THRESHOLD) < 0.17 and 0.012 < np.mean(err > 2 * THRESHOLD) < 0.020


def test_a_cap_of_a_quarter_and_a_floor_of_63_pixels(sim):
    q, truth = sim["quarter"], sim["truth"]
    assert max(q["lengths"]) == N // 4 and q["lengths"][:3] == [N // 4] * 3 and q["above"][-1] == 0
    adaptive = float(((ref.resolve(q["S"], q["counts"]).astype(np.float64) - truth) ** 2).mean())
    print(f"cap 0.25: {len(q['lengths'])} rounds, {q['samples'] / N:.1f} spp, MSE {adaptive:.4g}")
    assert abs(q["samples"] / N - 37.7) < 0.05 and abs(adaptive - 3.986e-4) < 1e-7
    m = sim["min63"]
    assert len(m["lengths"]) < ROUNDS and m["above"][-1] <= 63 < min(m["above"][:-1]) and m["lengths"] == sim["full"]["lengths"][:len(m["lengths"])]
