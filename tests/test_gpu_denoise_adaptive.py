"""The variance-guided filter with per-pixel sample counts on the device (pt_denoise_adaptive, csrc/pt_denoise.hip) against the
numpy restatement tests/denoise_adaptive_ref.py, bit for bit, in the adaptive and in the uniform state.  The restatement is always
fed with the GPU's own readbacks — image, feature buffers, noise planes and counts, each pinned by other tests — so these tests
isolate the filter.  Then: what stays untouched, what is refused, and what the filter buys on an adaptively sampled image."""
import numpy as np
import pytest

import denoise_adaptive_ref as aref
import denoise_guided_ref as gref
import denoise_ref as ref
from denoise_ref import bits, f32

pytestmark = pytest.mark.gpu
RES = (97, 61)
G = 3            # iterations per group and per round
ROUNDS = 3
FRACTION = 0.25
LAST = (2 + ROUNDS) * G  # the highest iteration number used
_CASES = {}


def pack_planes(f):
    """readback_features()'s dict back into the SUM planes [3, n, 4] the filter reads."""
    n = f["hits"].shape[0]
    planes = np.zeros((3, n, 4), f32)
    planes[0, :, :3], planes[0, :, 3] = f["normal"], f["depth"]
    planes[1, :, :3], planes[1, :, 3] = f["albedo"], f["hits"]
    planes[2, :, :3], planes[2, :, 3] = f["position"], f["object_id"].view(f32)
    return planes


def same(got, want, what):
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:2]], want[bad[:2]])


def render_groups(r, sizes, first=1):
    for n in sizes:
        r.render(first, n)
        r.noise_fold()
        first += n


def to_adaptive_state(r, rounds=ROUNDS):
    """Two folded groups of G, `rounds` rounds of G over FRACTION of the pixels."""
    render_groups(r, [G, G])
    for k in range(rounds):
        r.adaptive_round(1 + (2 + k) * G, G, FRACTION)


def readbacks(r):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    return r.readback(), pack_planes(r.readback_features()), capi.join_noise(r.readback_noise()), r.readback_adaptive()


def gpu_case(path, res, option_sets, **kw):
    """The adaptive state of to_adaptive_state and LAST feature iterations, anti-aliased, then one filter call per option set:
    (image SUM, feature planes, noise planes, counts, outputs)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    key = (path, tuple(res), repr(option_sets), tuple(sorted(kw.items())))
    if key not in _CASES:
        r = capi.Renderer(capi.Scene(path, res=res), aa_jitter=True, iters_per_batch=G, **kw)
        try:
            to_adaptive_state(r)
            r.render_features(1, LAST)
            _CASES[key] = readbacks(r) + ([r.denoise_adaptive(**o) for o in option_sets],)
        finally:
            r.free()
    return _CASES[key]


WHOLE = [dict(levels=1), dict(levels=3), dict(levels=5), dict(levels=5, keep_albedo=True)]


# ---- 6 .. 9: the adaptive state against the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(WHOLE)))
def test_adaptive_state_equals_restatement(scene_dir, k):
    img, planes, noise, counts, outs = gpu_case(scene_dir["cornell"], RES, WHOLE)
    hits, var = planes[1, :, 3], noise[0, :, 3]
    assert np.unique(counts[:, 0]).size >= 3 and counts[:, 1].min() >= 2
    assert (hits > 0).any() and (hits == 0).any()
    assert (var == 0).any() and (var > 0).sum() >= 1000  # misses and emitters beside noisy pixels
    assert np.array_equal(bits(noise[0, :, :3]), bits(img))  # the merge keeps prev == S
    stats = {}
    same(outs[k], aref.denoise_adaptive(img, planes, noise, counts, RES[0], RES[1], stats=stats, **WHOLE[k]), WHOLE[k])
    assert stats["cut"] > 0


@pytest.mark.parametrize("arith", ["fma", "fast"])
def test_modes_equal_restatement_of_their_own_readback(scene_dir, arith):
    img, planes, noise, counts, outs = gpu_case(scene_dir["cornell"], RES, [dict()], arith=arith)
    assert np.unique(counts[:, 0]).size >= 3
    same(outs[0], aref.denoise_adaptive(img, planes, noise, counts, RES[0], RES[1]), arith)


def test_contiguous_rows_tile(scene_dir):
    img, planes, noise, counts, outs = gpu_case(scene_dir["cornell"], RES, [dict()], pixel_begin=97 * 7, pixel_count=97 * 20)
    assert outs[0].shape == (97 * 20, 3) and np.unique(counts[:, 0]).size >= 3
    same(outs[0], aref.denoise_adaptive(img, planes, noise, counts, 97, 20), "rows 7 .. 26 as an image of their own")


def test_frame_smaller_than_a_workgroup_and_the_stencil(scene_dir):
    res = (33, 9)
    img, planes, noise, counts, outs = gpu_case(scene_dir["cornell"], res, [dict(levels=5)])
    assert (planes[1, :, 3] > 0).any() and (planes[1, :, 3] == 0).any() and np.unique(counts[:, 0]).size >= 2
    same(outs[0], aref.denoise_adaptive(img, planes, noise, counts, res[0], res[1], levels=5), res)


# ---- 10: the uniform state ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[2, 2, 2, 2], [2, 2, 2]], ids=["T8", "T6"])
def test_uniform_state(scene_dir, sizes):
    """T = 8: the multiplication and the division by Tf are exact, the result is pt_denoise_guided's bit for bit.  T = 6: the
    restatement's, with the counts pt_readback_adaptive reports."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    M, T = len(sizes), sum(sizes)
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=RES), aa_jitter=True)
    try:
        render_groups(r, sizes)
        r.render_features(1, T)
        img, planes, noise, counts = readbacks(r)
        assert np.array_equal(counts, aref.uniform_counts(RES[0] * RES[1], T, M))
        got, guided = r.denoise_adaptive(), r.denoise_guided()
    finally:
        r.free()
    assert (noise[0, :, 3] > 0).sum() >= 1000
    same(got, aref.denoise_adaptive(img, planes, noise, counts, RES[0], RES[1]), sizes)
    if T == 8:
        same(got, guided, "pt_denoise_guided")
    else:
        assert (bits(got) != bits(guided)).any()  # (a few roundings of var_0 apart)


# ---- 11: the stage entry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,rows", ref.FRAMES[:3])
def test_stage_equals_host(scene_dir, w, rows):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    groups, iters = 3, 7
    _, planes = ref.random_frame(w, rows, iters)
    noise = gref.random_noise_planes(w, rows, groups, iters)
    rgb = np.ascontiguousarray(noise[0, :, :3])
    counts = aref.random_counts(w, rows)
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(32, 24)))
    try:
        for opts in (dict(), dict(levels=8), dict(levels=3, keep_albedo=True), dict(sigma_color=-1.0), dict(sigma_color=3.0, sigma_normal=-1.0)):
            same(r.stage_denoise_adaptive(rgb, planes, noise, counts, w, rows, **opts), capi.denoise_adaptive_host(rgb, planes, noise, counts, w, rows, **opts),
                 (w, rows, opts))
        bad = counts.copy()
        bad[-1] = (1, 1)
        with pytest.raises(capi.PtError, match="pt_stage_denoise_adaptive: pixel %d .*M = 1" % (w * rows - 1)):
            r.stage_denoise_adaptive(rgb, planes, noise, bad, w, rows)
        with pytest.raises(capi.PtError, match="pt_stage_denoise_adaptive: .*levels"):
            r.stage_denoise_adaptive(rgb, planes, noise, counts, w, rows, levels=9)
    finally:
        r.free()


# ---- 12: nothing else moves -------------------------------------------------------------------------------------------------------
def test_nothing_else_moves(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = RES[0] * RES[1]
    scene = capi.Scene(scene_dir["cornell"], res=RES)
    for first_kind in ("adaptive", "unguided"):
        r = capi.Renderer(scene, aa_jitter=True, iters_per_batch=G)
        try:
            render_groups(r, [G, G])
            r.render_features(1, LAST)
            start = r.stats().device_bytes
            if first_kind == "unguided":  # (still the uniform state: pt_denoise allocates the shared workspace)
                r.denoise(2 * G)
                assert r.stats().device_bytes == start + 80 * n
            for k in range(ROUNDS):
                r.adaptive_round(1 + (2 + k) * G, G, FRACTION)
            state = readbacks(r)
            before, est = r.stats(), r.noise()
            first = r.denoise_adaptive()
            after = r.stats()
            assert after.device_bytes == before.device_bytes + (80 * n if first_kind == "adaptive" else 0) and after.samples == before.samples
            again = r.denoise_adaptive(levels=2)
            assert r.stats().device_bytes == after.device_bytes
            assert (bits(again) != bits(first)).any()
            same(r.denoise_adaptive(), first, "a second call")
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(readbacks(r), state))
            assert r.noise() == est and r.stats().samples == before.samples
            with pytest.raises(capi.PtError, match="adaptive state"):  # the other two filters keep refusing it
                r.denoise_guided()
            with pytest.raises(capi.PtError, match="adaptive state"):
                r.denoise(LAST)
        finally:
            r.free()
    _, _, _, _, outs = gpu_case(scene_dir["cornell"], RES, WHOLE)
    same(first, outs[2], "the shared case")


def test_a_round_after_a_filter_call_is_the_round_it_would_have_been(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(scene_dir["cornell"], res=RES)
    ends = []
    for filtered in (False, True):
        r = capi.Renderer(scene, aa_jitter=True, iters_per_batch=G)
        try:
            to_adaptive_state(r, rounds=2)
            r.render_features(1, 4 * G)
            if filtered:
                r.denoise_adaptive()
            r.adaptive_round(1 + 4 * G, G, FRACTION)
            ends.append((r.readback(), capi.join_noise(r.readback_noise()), r.readback_adaptive(), r.stats().samples))
        finally:
            r.free()
    plain, with_call = ends
    assert all(np.array_equal(bits(a) if a.dtype == f32 else a, bits(b) if b.dtype == f32 else b) for a, b in zip(plain[:3], with_call[:3]))
    assert plain[3] == with_call[3] and np.unique(plain[2][:, 0]).size >= 3


# ---- 13: refusals ----------------------------------------------------------------------------------------------------------------
def test_errors(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    sc = capi.Scene(scene_dir["cornell"], res=RES)
    r = capi.Renderer(sc, pixel_begin=97 * 7, pixel_count=97 * 20, stripe_pixels=97, stripe_stride=194)
    try:
        render_groups(r, [1, 1])
        r.render_features(1, 2)
        before = r.stats().device_bytes
        with pytest.raises(capi.PtError, match="pt_denoise_adaptive: .*whole contiguous image rows"):
            r.denoise_adaptive()
        assert r.stats().device_bytes == before
    finally:
        r.free()
    r = capi.Renderer(sc)
    try:
        r.render(1, 1)
        before = r.stats().device_bytes
        with pytest.raises(capi.PtError, match="pt_denoise_adaptive: no feature pass"):
            r.denoise_adaptive()
        assert r.stats().device_bytes == before
        r.render_features(1, 1)
        before = r.stats().device_bytes
        with pytest.raises(capi.PtError, match="pt_denoise_adaptive: nothing has been folded"):
            r.denoise_adaptive()
        assert r.stats().device_bytes == before
        r.noise_fold()
        before = r.stats().device_bytes
        with pytest.raises(capi.PtError, match="pt_denoise_adaptive: 1 group.*at least 2"):
            r.denoise_adaptive()
        r.render(2, 1)
        r.noise_fold()
        r.render(3, 1)
        with pytest.raises(capi.PtError, match="pt_denoise_adaptive: .*fold first"):
            r.denoise_adaptive()
        r.noise_fold()
        for bad, match in ((dict(levels=9), "levels"), (dict(sigma_normal=float("nan")), "sigma")):
            with pytest.raises(capi.PtError, match="pt_denoise_adaptive: .*" + match):
                r.denoise_adaptive(**bad)
        assert r.stats().device_bytes == before  # a refused call allocates nothing
        assert r.denoise_adaptive().shape == (RES[0] * RES[1], 3)
        r.adaptive_round(4, 1, FRACTION)
        for bad, match in ((dict(levels=9), "levels"), (dict(sigma_color=float("nan")), "sigma")):  # ... in the adaptive state too
            with pytest.raises(capi.PtError, match="pt_denoise_adaptive: .*" + match):
                r.denoise_adaptive(**bad)
        assert r.denoise_adaptive().shape == (RES[0] * RES[1], 3)
        r.clear()
        before = r.stats().device_bytes
        with pytest.raises(capi.PtError, match="pt_denoise_adaptive: nothing has been folded"):
            r.denoise_adaptive()
        assert r.stats().device_bytes == before
    finally:
        r.free()


# ---- 14: what it buys --------------------------------------------------------------------------------------------------------------
SIMULATED_B_OVER_A = 0.1648


def test_what_it_buys(scene_dir):
    """Cornell 96x54, depth 8, exact, against 2048 spp (iterations 100001 ...), the configuration of test_gpu_adaptive.py's benefit
    test: two uniform groups of 4, then 24 rounds of 4 over the noisiest quarter (32 iterations' worth of samples), features over
    the 104 iteration numbers used.  MSE of (a) the resolved adaptive image, (b) pt_denoise_adaptive of it, (c) 32 uniform
    iterations folded in four groups of 8 and filtered by pt_denoise_guided; all filters at their defaults.
    Simulated on the CPU (the oracle's samples, which the exact build reproduces, with pt_noise_fold_host, pt_adaptive_select_host,
    pt_adaptive_merge_host, pt_denoise_adaptive_host and pt_denoise_guided_host): a 4.90261e-4, b 8.07958e-5, c 1.29435e-4;
    b / a = 0.1648, b / c = 0.6242.  The bound on b / a is min(1, 1.25 x simulated) = 0.2060, the 25 % being head-room for a later
    retuning of defaults and for nothing else; b / c is recorded, not asserted.
    Measured on an MI355X: a 4.90261e-4, b 8.07958e-5, c 1.29435e-4; b / a = 0.1648, b / c = 0.6242 (the simulation's digits: the exact
    build reproduces the oracle's samples bit for bit, and the filter is specified to the bit)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res = (96, 54)
    n = res[0] * res[1]
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=res), arith="exact")
    try:
        assert r.scene.trace_depth == 8
        r.render(100001, 2048)
        truth = r.readback().astype(np.float64) / 2048

        def mse(x):
            return float(np.mean((x.astype(np.float64) - truth) ** 2))
        r.clear()
        render_groups(r, [8, 8, 8, 8])
        r.render_features(1, 32)
        c = mse(r.denoise_guided())
        r.clear()  # (the feature buffers are cleared with the image)
        max_iters = 8 + 4 * 24
        done, samples, _ = r.render_adaptive(1, max_iters, target_db=200.0, fraction=0.25, group_iters=4)
        assert (done, samples) == (max_iters, 32 * n)
        r.render_features(1, max_iters)
        hits = r.readback_features()["hits"]
        assert hits.max() == max_iters  # one feature pass, of this render
        a, b = mse(r.resolve()), mse(r.denoise_adaptive())
    finally:
        r.free()
    print(f"what the adaptive filter buys: MSE raw adaptive {a:.6g}, filtered adaptive {b:.6g}, filtered uniform {c:.6g}; b / a {b / a:.4f} "
          f"(simulated {SIMULATED_B_OVER_A}), b / c {b / c:.4f} (simulated 0.6242)")
    assert b < a
    assert b / a <= min(1.0, 1.25 * SIMULATED_B_OVER_A), (b / a, SIMULATED_B_OVER_A)
