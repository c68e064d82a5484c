"""Adaptive sampling by threshold on the device (pt_adaptive_round_threshold, pt_render_threshold; csrc/pt_adaptive.hip and the
worker context of csrc/pt_post.cpp, planned once for a capacity and run at any live length) against the numpy restatement
tests/adaptive_threshold_ref.py, bit for bit; what it buys against uniform sampling; and what it refuses."""
import numpy as np
import pytest

import adaptive_ref as ref
import adaptive_threshold_ref as tref
from adaptive_ref import bits, f32

pytestmark = pytest.mark.gpu
G = 3  # iterations per group and per round of the made-up runs


def raw_planes(r):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    out = np.empty((2, r.n, 4), f32)
    capi._check(capi.lib().pt_readback_noise(capi._f(out)))
    return out


def warm_up(r, groups=2, n=G, first=1):
    for j in range(groups):
        r.render(first + j * n, n)
        r.noise_fold()


# ---- (a) one worker, planned for a capacity, at live lengths that shrink and grow again ----------------------------------------
CAPACITY_RES = (97, 11)          # 1067 pixels: 17 chunks of 64, the last one partial
LIVE = (1067, 65, 64, 63, 1, 500, 1067)
ITERS = 7                        # with iters_per_batch = 3: two full batches and a cut one


def capacity_check(scene_dir, **kw):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = CAPACITY_RES[0] * CAPACITY_RES[1]
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=CAPACITY_RES), iters_per_batch=3, **kw)
    try:
        r.render(1, ITERS)
        plain = r.readback()
        assert np.isfinite(plain).all() and plain.max() > 0
        rng = np.random.default_rng(11)
        with_worker = None
        for step, m in enumerate(LIVE):
            lst = np.sort(rng.choice(n, m, replace=False)).astype(np.int32) if step % 3 else rng.permutation(n)[:m].astype(np.int32)
            got = capi.stage_render_list_capacity(lst, n, 1, ITERS)
            bad = np.flatnonzero((bits(got) != bits(plain[lst])).any(axis=1))
            assert bad.size == 0, (kw, step, m, bad.size, lst[bad[:4]], got[bad[:2]], plain[lst[bad[:2]]])
            if with_worker is None:
                with_worker = r.stats().device_bytes
            assert r.stats().device_bytes == with_worker, (kw, step, m)  # ONE worker: nothing allocated or freed after the first call
        assert np.array_equal(bits(r.readback()), bits(plain))  # the renderer's own image is untouched
    finally:
        r.free()


@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
@pytest.mark.parametrize("aa_jitter", [True, False], ids=["jitter", "shared"])
def test_worker_at_capacity_equals_rows_of_the_plain_image(scene_dir, arith, aa_jitter):
    capacity_check(scene_dir, arith=arith, aa_jitter=aa_jitter)


def test_worker_at_capacity_with_split_records(scene_dir):
    capacity_check(scene_dir, debug_flags=8192)  # no first bounce in k_paths: split records, records by visit, the tile gather


def test_capacity_stage_refuses(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(33, 9)), iters_per_batch=3)
    try:
        before = r.stats().device_bytes
        for lst, capacity in (([0, 1, 2], 2), ([0], 33 * 9 + 1), ([0], 0)):
            with pytest.raises(capi.PtError, match="bad argument"):
                capi.stage_render_list_capacity(np.array(lst, np.int32), capacity, 1, 1)
        assert r.stats().device_bytes == before
    finally:
        r.free()


# ---- (b) whole rounds against the restatement -----------------------------------------------------------------------------------
RES = (97, 61)
N = RES[0] * RES[1]
CAP_FRACTION = 0.25


def threshold_for(planes, counts, want_above):
    """A threshold that leaves about want_above pixels above: the square root, rounded down a little, of the key at that rank."""
    k = np.sort(ref.keys(planes[0, :, 3], RES[0], RES[1], counts).view(f32))[::-1]
    return float(np.sqrt(np.float64(k[want_above]))) * (1 + 1e-6)


@pytest.mark.parametrize("arith, aa_jitter", [("exact", False), ("fast", True)], ids=["exact-shared", "fast-jitter"])
def test_rounds_equal_restatement(scene_dir, arith, aa_jitter):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(scene_dir["cornell"], res=RES)
    kw = dict(arith=arith, aa_jitter=aa_jitter, iters_per_batch=G)
    rounds = 7  # groups of iterations handed to a round, those that select nothing included
    # the image of every iteration of the rounds from a plain renderer; a worker starts its group sum at zero and the gather adds a
    # pixel's samples in iteration order (tests/test_gpu_adaptive.py)
    plain = capi.Renderer(scene, **kw)
    try:
        group_sum = []
        for j in range(2, 2 + rounds):
            total = np.zeros((N, 3), f32)
            for i in range(1 + j * G, 1 + (j + 1) * G):
                plain.clear()
                plain.render(i, 1)
                total = (total + plain.readback()).astype(f32)
            group_sum.append(total)
    finally:
        plain.free()
    cap = ref.list_length(CAP_FRACTION, N)
    r = capi.Renderer(scene, **kw)
    try:
        warm_up(r)
        S, planes = r.readback(), raw_planes(r)
        counts = ref.uniform_counts(N, 2 * G, 2)
        done, samples, lengths = 0, 2 * G * N, []

        def same_state(what):
            got_S, got_planes, got_counts = r.readback(), raw_planes(r), r.readback_adaptive()
            assert np.array_equal(got_counts, counts), (what, np.flatnonzero((got_counts != counts).any(axis=1))[:8])
            bad = np.flatnonzero((bits(got_S) != bits(S)).any(axis=1))
            assert bad.size == 0, (what, bad.size, bad[:8], got_S[bad[:2]], S[bad[:2]])
            bad = np.flatnonzero((bits(got_planes) != bits(planes)).reshape(2, N, 4).any(axis=(0, 2)))
            assert bad.size == 0, (what, bad.size, bad[:8])
            assert np.array_equal(bits(r.resolve()), bits(ref.resolve(S, counts))), what
            assert r.stats().samples == samples, what

        # a list cut by the cap; four lists that shrink, the last a handful of pixels; nothing above; and a cut list again
        for k, want_above in enumerate((None, cap // 2, cap // 8, 70, 3, -1, None)):
            threshold = 0.0 if want_above is None else 1e3 if want_above < 0 else threshold_for(planes, counts, want_above)
            lst, above, m = tref.select_threshold(planes[0, :, 3], RES[0], RES[1], counts, threshold, cap)
            what = (arith, aa_jitter, k, threshold, above, m)
            before = r.noise()
            got = r.adaptive_round_threshold(1 + (2 + k) * G, G, threshold, CAP_FRACTION)
            assert got == (above, m), (what, got)
            if want_above is None:
                assert above > cap == m
            elif want_above < 0:
                assert (above, m) == (0, 0) and r.noise() == before  # no round counted, SSE_est where it was
            else:
                assert 0 < above == m < cap and (not lengths or m < lengths[-1]), (what, lengths)
            if m:
                want_sse = ref.merge(S, planes, counts, lst, group_sum[k][lst], G)
                done, samples = done + 1, samples + G * m
                lengths.append(m)
                noise = r.noise()
                assert (noise["groups"], noise["iterations"]) == (2 + done, (3 + k) * G), (what, noise)
                assert want_sse > 0 and abs(noise["sse"] - want_sse) <= 1e-9 * want_sse, (what, noise["sse"], want_sse)
            same_state(what)
        assert done == 6 and lengths[0] == lengths[-1] == cap and min(lengths) <= 4
        # ... and a fixed-fraction round on the same renderer, on the same worker: its live size is the capacity again
        bytes_before = r.stats().device_bytes
        lst = ref.select(planes[0, :, 3], RES[0], RES[1], counts, cap)
        ref.merge(S, planes, counts, lst, group_sum[5][lst], G)  # (the iterations of the round that selected nothing)
        r.adaptive_round(1 + 7 * G, G, CAP_FRACTION)
        samples += G * cap
        same_state("fixed fraction after threshold rounds")
        assert r.stats().device_bytes == bytes_before and r.noise()["groups"] == 2 + done + 1
    finally:
        r.free()


# ---- (c) the driver in the simulated configuration ---------------------------------------------------------------------------------
def test_render_threshold_reproduces_the_simulation(scene_dir):
    """Cornell 96x54, depth 8, exact: two uniform groups of 4, then threshold rounds of 4 at 0.05 with cap fraction 1, against 4096
    spp (iterations 100001 ...).  The exact build reproduces the oracle's samples and everything after them is specified to the bit,
    so the run must equal the restatement on the renderer's own samples in rounds, samples, per-round list lengths and the resolved
    image — and with them tests/test_adaptive_threshold_sim.py's figures: 84 rounds, 200,160 samples, MSE ratio 0.484 against
    uniform sampling at equal samples (bound 0.75, the head-room of test_gpu_adaptive.py's benefit test), 0.112 of the samples
    uniform sampling needs for the criterion (bound 0.25: uniform's figure hangs on its single worst pixel)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res, Gs, threshold = (96, 54), 4, 0.05
    n = res[0] * res[1]
    scene = capi.Scene(scene_dir["cornell"], res=res)
    plain = capi.Renderer(scene, arith="exact")
    try:
        assert plain.scene.trace_depth == 8
        plain.render(100001, 4096)
        truth = plain.readback().astype(np.float64) / 4096
        cache = {}

        def group_sum(first, count, accum=None):
            """Iterations first .. of every pixel from zero, or (accum: the sum of iterations 1 .. first - 1) continuing it: the
            gather adds a pixel's samples one by one in iteration order, so that is the sum of iterations 1 .. first + count - 1."""
            key = (first, count) if accum is None else (1, first - 1 + count)
            if key not in cache:
                plain.clear()
                plain.render(*key)
                cache[key] = plain.readback()
            return cache[key]

        sim = tref.simulate(res[0], res[1], group_sum, Gs, threshold, 1.0, 400)
        sim63 = tref.simulate(res[0], res[1], group_sum, Gs, threshold, 1.0, 400, min_pixels=63)
        uniform_groups, uniform_sums = tref.uniform_groups_to_criterion(res[0], res[1], group_sum, Gs, threshold, 120)
    finally:
        plain.free()
    rounds = len(sim["lengths"])
    want_image = ref.resolve(sim["S"], sim["counts"])

    r = capi.Renderer(scene, arith="exact")
    try:
        done, samples, above_left = r.render_threshold(1, 2 * Gs + 400 * Gs, threshold, max_fraction=1.0, group_iters=Gs)
        image, counts, noise = r.resolve(), r.readback_adaptive(), r.noise()
        assert (done, samples, above_left) == (2 * Gs + rounds * Gs, sim["samples"], 0) and r.stats().samples == samples
        assert (noise["groups"], noise["iterations"]) == (2 + rounds, done)
        assert np.array_equal(counts, sim["counts"]) and np.array_equal(bits(image), bits(want_image))
        assert np.array_equal(bits(raw_planes(r)), bits(sim["planes"]))
        # the same run round by round: the per-round list lengths
        r.clear()
        warm_up(r, n=Gs)
        lengths, k = [], 0
        while True:
            above, m = r.adaptive_round_threshold(1 + (2 + k) * Gs, Gs, threshold, 1.0)
            assert above == m == sim["above"][k], (k, above, m)
            if m == 0:
                break
            lengths.append(m)
            k += 1
        assert lengths == sim["lengths"] and np.array_equal(bits(r.resolve()), bits(want_image))
        # a floor of 63 pixels ends earlier
        r.clear()
        done63, samples63, left63 = r.render_threshold(1, 2 * Gs + 400 * Gs, threshold, max_fraction=1.0, group_iters=Gs, min_pixels=63)
        assert done63 < done and left63 <= 63 and (done63, samples63, left63) == (2 * Gs + len(sim63["lengths"]) * Gs, sim63["samples"], sim63["above"][-1])
        assert np.array_equal(bits(r.resolve()), bits(ref.resolve(sim63["S"], sim63["counts"])))
    finally:
        r.free()
    groups = samples // (Gs * n)  # the uniform groups the adaptive samples pay for
    mse_adaptive = float(((image.astype(np.float64) - truth) ** 2).mean())
    mse_uniform = float(((uniform_sums[groups - 1].astype(np.float64) / (groups * Gs) - truth) ** 2).mean())
    needs = (uniform_groups if uniform_groups else len(uniform_sums)) * Gs * n  # (not met within 120 groups: at least those)
    print(f"threshold {threshold}: {rounds} rounds, {samples} samples = {samples / n:.1f} spp, lists {lengths[:3]} ... {lengths[-4:]}, max T {counts[:, 0].max()}; "
          f"MSE {mse_adaptive:.4g} against uniform's {mse_uniform:.4g} at {groups * Gs} spp, ratio {mse_adaptive / mse_uniform:.4f}; uniform meets the criterion "
          f"after {uniform_groups} groups, samples ratio {samples / needs:.4f}; min_pixels 63: {done63} iterations, {samples63} samples, {left63} left")
    assert (rounds, samples) == (84, 200_160), "the simulation's figures (tests/test_adaptive_threshold_sim.py)"
    assert mse_adaptive <= 0.75 * mse_uniform, (mse_adaptive, mse_uniform)
    assert samples <= 0.25 * needs, (samples, needs)


# ---- (d) refusals, and what stays as it was ---------------------------------------------------------------------------------------
def test_refusals_allocate_nothing(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res = (33, 9)
    scene = capi.Scene(scene_dir["cornell"], res=res)

    def refused(r, match, *args, call="adaptive_round_threshold"):
        before = r.stats().device_bytes
        with pytest.raises(capi.PtError, match=match):
            getattr(r, call)(*args)
        assert r.stats().device_bytes == before, match

    r = capi.Renderer(scene, iters_per_batch=G)
    try:
        refused(r, "0 group", 1, G, 0.1, 0.25)
        r.render(1, G)
        r.noise_fold()
        refused(r, "1 group", 1 + G, G, 0.1, 0.25)
        r.render(1 + G, G)
        r.noise_fold()
        r.render(1 + 2 * G, G)
        refused(r, "fold first", 1 + 3 * G, G, 0.1, 0.25)
        r.noise_fold()
        for fraction in (0.0, -0.25, 1.5, float("nan")):
            refused(r, "fraction", 1 + 3 * G, G, 0.1, fraction)
        refused(r, "at least one", 1 + 3 * G, 0, 0.1, 0.25)
        refused(r, "first is >= 1", 0, G, 0.1, 0.25)
        for threshold in (-0.1, float("nan"), float("inf")):
            refused(r, "threshold", 1 + 3 * G, G, threshold, 0.25)
            refused(r, "threshold", 1 + 3 * G, 10, threshold, 0.25, call="render_threshold")
        refused(r, "fraction", 1 + 3 * G, G, float("nan"), 0.0)  # the order of pt_adaptive_round's refusals first
        refused(r, "fraction", 1 + 3 * G, 10, 0.1, 0.0, call="render_threshold")
        refused(r, "pixels >= 0", 1 + 3 * G, 10, 0.1, 0.25, 0, -1, call="render_threshold")
        refused(r, "count is >= 1", 1 + 3 * G, 0, 0.1, 0.25, call="render_threshold")
        assert r.noise()["groups"] == 3 and np.array_equal(r.readback_adaptive(), ref.uniform_counts(res[0] * res[1], 3 * G, 3))  # still the uniform state
        before = r.stats().device_bytes
        above, m = r.adaptive_round_threshold(1 + 3 * G, G, 1e3, 0.25)  # selects nothing, and still enters the adaptive state
        assert (above, m) == (0, 0) and r.stats().device_bytes > before and r.noise()["groups"] == 3
        with pytest.raises(capi.PtError, match=r"adaptive state.*pt_resolve.*pt_clear"):
            r.render(1 + 3 * G, 1)
    finally:
        r.free()
    for kw, match in ((dict(pixel_begin=33, pixel_count=33 * 4, stripe_pixels=33, stripe_stride=66), "whole contiguous image rows"),
                      (dict(pixel_begin=5, pixel_count=33 * 3 + 7), "whole contiguous image rows"),
                      (dict(convergence=2), "convergence")):
        r = capi.Renderer(scene, iters_per_batch=G, **kw)
        try:
            warm_up(r)
            refused(r, match, 1 + 2 * G, G, 0.1, 0.25)
            refused(r, match, 1 + 2 * G, 10, 0.1, 0.25, call="render_threshold")
        finally:
            r.free()


def test_a_renderer_without_threshold_rounds_allocates_what_it_did_and_clear_returns_to_uniform(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(scene_dir["cornell"], res=RES)
    kw = dict(aa_jitter=True, iters_per_batch=G)

    def uniform_run(r):
        warm_up(r)
        return r.readback(), raw_planes(r), r.noise(), r.readback_adaptive()

    def fixed_rounds(r):
        warm_up(r)
        r.adaptive_round(1 + 2 * G, G, CAP_FRACTION)
        r.adaptive_round(1 + 3 * G, G, CAP_FRACTION)
        return r.readback(), raw_planes(r), r.noise(), r.readback_adaptive()

    fresh = capi.Renderer(scene, **kw)
    try:
        at_init = fresh.stats().device_bytes
        want_uniform = uniform_run(fresh)
        folded = fresh.stats().device_bytes
        assert folded == at_init + 32 * N + 8 * ((N + 1023) // 1024 + 1)  # the fold's state and nothing else (include/pt_amd.h)
        fresh.clear()
        want_fixed = fixed_rounds(fresh)
        fixed_bytes = fresh.stats().device_bytes
    finally:
        fresh.free()
    r = capi.Renderer(scene, **kw)
    try:
        warm_up(r)
        above, m = r.adaptive_round_threshold(1 + 2 * G, G, 0.0, CAP_FRACTION)
        assert above > m == ref.list_length(CAP_FRACTION, N)
        above, m = r.adaptive_round_threshold(1 + 3 * G, G, threshold_for(raw_planes(r), r.readback_adaptive(), 100), CAP_FRACTION)
        assert 0 < m == above < 200
        # the threshold rounds allocate what fixed-fraction rounds over the same fraction do: counts, workspace, list, one worker
        assert r.stats().device_bytes == fixed_bytes
        r.clear()
        assert r.stats().device_bytes == fixed_bytes and r.noise() == dict(sse=-1.0, groups=0, iterations=0) and not r.readback_adaptive().any()
        for run, want in ((uniform_run, want_uniform), (fixed_rounds, want_fixed)):
            for a, b in zip(run(r), want):
                assert a == b if isinstance(a, dict) else np.array_equal(a.view(np.uint32), b.view(np.uint32)), run.__name__
            r.clear()
        assert r.stats().device_bytes == fixed_bytes  # the fixed-fraction rounds ran on the worker the threshold rounds left, shrunk
    finally:
        r.free()
