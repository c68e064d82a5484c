"""The noise estimate on the device (pt_noise_fold, csrc/pt_noise.hip) against the numpy restatement tests/noise_ref.py, bit for
bit, and render_until built on it.  The restatement is always fed with the GPU's own readback() — pinned to the oracle by other
tests — so these tests isolate the fold."""
import numpy as np
import pytest

import noise_ref as ref
from noise_ref import bits, f32

pytestmark = pytest.mark.gpu
RES = (97, 61)
GROUPS = (3, 1, 4, 2)
_CASES = {}


def state_bytes(n):
    return 32 * n + 8 * ((n + 1023) // 1024 + 1)  # include/pt_amd.h


def raw_planes(r):
    """pt_readback_noise's planes as they are: [2, n, 4]."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    out = np.empty((2, r.n, 4), f32)
    capi._check(capi.lib().pt_readback_noise(capi._f(out)))
    return out


def psnr(sse, pixels):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    return capi.psnr_from_sse(sse, pixels)


def run_groups(r, groups, first=1):
    """render + fold per group: [(SUM image, planes, noise())] after every fold."""
    out, it = [], first
    for n in groups:
        r.render(it, n)
        it += n
        r.noise_fold()
        out.append((r.readback(), raw_planes(r), r.noise()))
    return out


def gpu_case(path, res, groups, **kw):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    key = (path, tuple(res), tuple(groups), tuple(sorted(kw.items())))
    if key not in _CASES:
        r = capi.Renderer(capi.Scene(path, res=res), aa_jitter=True, **kw)
        try:
            _CASES[key] = run_groups(r, groups)
        finally:
            r.free()
    return _CASES[key]


def check_against_restatement(steps, groups, what):
    npix = steps[0][0].shape[0]
    want, T = ref.new_planes(npix), 0
    for M, (n, (S, planes, noise)) in enumerate(zip(groups, steps), start=1):
        T += n
        w, _ = ref.fold(S, want, n, M, T)
        bad = np.flatnonzero((bits(planes) != bits(want)).reshape(2, npix, 4).any(axis=(0, 2)))
        assert bad.size == 0, (what, M, bad.size, bad[:8], planes[:, bad[:2]], want[:, bad[:2]])
        assert (noise["groups"], noise["iterations"]) == (M, T)
        if M < 2:
            assert noise["sse"] == -1.0
        else:
            exact = float(np.sum(w.astype(np.float64)))
            assert exact > 0 and abs(noise["sse"] - exact) <= 1e-9 * exact, (what, M, noise["sse"], exact)


TILES = {
    "whole": dict(),
    "striped": dict(pixel_begin=97 * 7, pixel_count=97 * 20, stripe_pixels=97, stripe_stride=194),
    "ragged": dict(pixel_begin=50, pixel_count=97 * 20 + 13),  # contiguous, no whole rows, 1953 pixels: two workgroups, the second partly empty
    "fifty": dict(pixel_begin=1000, pixel_count=50),           # less than a wave
}


@pytest.mark.parametrize("tile", sorted(TILES))
def test_planes_equal_restatement(scene_dir, tile):
    steps = gpu_case(scene_dir["cornell"], RES, GROUPS, iters_per_batch=3, **TILES[tile])
    assert steps[-1][1][0, :, 3].max() > 0  # some pixel is noisy
    check_against_restatement(steps, GROUPS, tile)


@pytest.mark.parametrize("arith", ["fma", "fast"])
def test_modes_equal_restatement_of_their_own_readback(scene_dir, arith):
    check_against_restatement(gpu_case(scene_dir["cornell"], RES, GROUPS, iters_per_batch=3, arith=arith), GROUPS, arith)


def test_frame_smaller_than_a_workgroup(scene_dir):
    check_against_restatement(gpu_case(scene_dir["cornell"], (33, 9), GROUPS, iters_per_batch=3), GROUPS, "33x9")


def test_fold_semantics(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = RES[0] * RES[1]
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=RES), aa_jitter=True, iters_per_batch=3)
    try:
        before = r.stats().device_bytes
        r.noise_fold()  # nothing rendered: nothing to fold, nothing allocated
        assert r.noise() == dict(sse=-1.0, groups=0, iterations=0) and r.stats().device_bytes == before
        with pytest.raises(capi.PtError, match="nothing has been folded"):
            r.readback_noise()
        r.render(1, 2)
        r.render(3, 3)
        r.reset_stats()  # zeroes PtStats.samples, not the count of rendered iterations
        r.noise_fold()  # both calls are ONE group of five
        S, planes = r.readback(), raw_planes(r)
        assert r.noise() == dict(sse=-1.0, groups=1, iterations=5)
        want = ref.new_planes(n)
        ref.fold(S, want, 5, 1, 5)
        assert np.array_equal(bits(planes), bits(want))
        r.noise_fold()  # nothing new
        assert r.noise() == dict(sse=-1.0, groups=1, iterations=5) and np.array_equal(bits(raw_planes(r)), bits(planes))
        r.render(6, 2)
        r.noise_fold()
        ref.fold(r.readback(), want, 2, 2, 7)
        assert np.array_equal(bits(raw_planes(r)), bits(want))
        named = r.readback_noise()
        assert np.array_equal(bits(named["prev"]), bits(want[0, :, :3])) and np.array_equal(bits(named["q"]), bits(want[1, :, :3]))
        assert np.array_equal(bits(named["variance"]), bits(want[0, :, 3]))
        two = r.noise()
        r.noise_fold()
        assert r.noise() == two and two["groups"] == 2 and two["sse"] > 0
    finally:
        r.free()


def test_noise_repeats_after_clear_and_nothing_else_moves(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = RES[0] * RES[1]
    steps = gpu_case(scene_dir["cornell"], RES, GROUPS, iters_per_batch=3)
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=RES), aa_jitter=True, iters_per_batch=3)
    try:
        it = 1
        for k in GROUPS:  # the same renders without a fold
            r.render(it, k)
            it += k
        plain, st = r.readback(), r.stats()
        assert np.array_equal(bits(plain), bits(steps[-1][0])) and st.samples == sum(GROUPS) * n
        r.clear()
        first = run_groups(r, GROUPS)
        after = r.stats()
        assert after.device_bytes == st.device_bytes + state_bytes(n) and after.samples == sum(GROUPS) * n
        assert np.array_equal(bits(first[-1][0]), bits(plain))
        r.clear()
        assert r.noise() == dict(sse=-1.0, groups=0, iterations=0) and not raw_planes(r).any()
        again = run_groups(r, GROUPS)
        assert r.stats().device_bytes == after.device_bytes  # allocated once
        for a, b, c in zip(first, again, steps):
            assert a[2] == b[2] == c[2], (a[2], b[2], c[2])  # equal bits of the double, too
            assert np.array_equal(bits(a[1]), bits(b[1]))
    finally:
        r.free()


def test_the_estimator_estimates(scene_dir):
    """The bound of tests/test_noise_host.py::test_the_estimator_estimates with the device's images and folds."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res, groups = (64, 48), [4] * 8
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=res), aa_jitter=True)
    try:
        r.render(100001, 2048)
        truth = r.readback().astype(np.float64) / 2048
        r.clear()
        steps = run_groups(r, groups)
    finally:
        r.free()
    ratios = []
    for M, (S, _, noise) in enumerate(steps, start=1):
        if M >= 2:
            ratios.append(noise["sse"] / float(np.sum((S.astype(np.float64) / (4 * M) - truth) ** 2)))
    print("SSE_est / actual at M = 2 ..:", [round(x, 4) for x in ratios])
    assert len(ratios) == 7 and all(2 / 3 <= x <= 3 / 2 for x in ratios), ratios


def test_render_until(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res = (64, 48)
    n = res[0] * res[1]
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=res), aa_jitter=True, iters_per_batch=3)
    try:
        manual = [psnr(s[2]["sse"], n) if s[2]["sse"] >= 0 else -1.0 for s in run_groups(r, [4] * 6)]
        print("estimated PSNR after groups 1 ..:", manual)
        target = 0.5 * (manual[3] + manual[4])  # between M = 4 and M = 5
        assert manual[0] == -1.0 and max(manual[1:4]) < target < manual[4], (manual, target)
        r.clear()
        done, db = r.render_until(1, 40, target, group_iters=4)
        assert done == 20 and f32(db).view(np.uint32) == f32(manual[4]).view(np.uint32), (done, db, manual)
        assert r.noise()["groups"] == 5 and r.noise()["iterations"] == 20 and r.stats().samples == 20 * n
        stopped = r.readback()
        r.clear()
        r.render(1, 20)
        assert np.array_equal(bits(stopped), bits(r.readback()))
        # a target out of reach: the cap, the last group cut to it
        r.clear()
        done, db = r.render_until(1, 10, 99.0, group_iters=4)
        got, noise = raw_planes(r), r.noise()
        assert done == 10 and (noise["groups"], noise["iterations"]) == (3, 10) and 0 < db < 99.0
        assert f32(db).view(np.uint32) == f32(psnr(noise["sse"], n)).view(np.uint32)
        r.clear()
        check_against_restatement(run_groups(r, (4, 4, 2)), (4, 4, 2), "4, 4, 2")
        assert np.array_equal(bits(raw_planes(r)), bits(got))
        # group_iters = 0: a batch (three iterations here)
        r.clear()
        done, _ = r.render_until(1, 7, 99.0)
        assert done == 7 and (r.noise()["groups"], r.noise()["iterations"]) == (3, 7)
        # a cap that one group reaches: no estimate
        r.clear()
        assert r.render_until(1, 2, 10.0, group_iters=5) == (2, -1.0)
    finally:
        r.free()


def test_group_equals_single_context(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path, res = scene_dir["cornell"], (96, 60)
    n = res[0] * res[1]
    single = gpu_case(path, res, [4] * 6)
    sse = [s[2]["sse"] for s in single]
    manual = [psnr(x, n) for x in sse[1:]]  # M = 2 ..
    target = 0.5 * (manual[2] + manual[3])  # between M = 4 and M = 5
    assert max(manual[:3]) < target < manual[3]
    g = capi.Group(capi.Scene(path, res=res), [0, 0, 0], aa_jitter=True)
    try:
        it = 1
        for M in range(1, 7):
            g.render(it, 4)
            it += 4
            g.noise_fold()
            got = g.noise()
            assert (got["groups"], got["iterations"]) == (M, 4 * M)
            if M < 2:
                assert got["sse"] == -1.0
            else:
                assert abs(got["sse"] - sse[M - 1]) <= 1e-9 * sse[M - 1], (M, got, sse[M - 1])
        for i in range(3):
            assert g.stats(i).samples == 24 * (n // 3)
        with pytest.raises(capi.PtError, match="pt_group_render_until"):
            g.render_until(0, 10, 30.0)
    finally:
        g.free()
    g = capi.Group(capi.Scene(path, res=res), [0, 0, 0], aa_jitter=True)
    try:
        done, db = g.render_until(1, 40, target, group_iters=4)
        assert done == 20 and abs(db - manual[3]) < 1e-3, (done, db, manual)
        assert np.array_equal(bits(g.gather()), bits(single[4][0]))
    finally:
        g.free()


@pytest.mark.parametrize("bad", [dict(iter_first=0), dict(max_iters=0), dict(max_iters=-3), dict(group_iters=-1), dict(target_db=float("nan")),
                                 dict(target_db=float("inf")), dict(iter_first=2**31 - 5, max_iters=10)])
def test_errors(scene_dir, bad):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(33, 9)))
    try:
        before = r.stats().device_bytes
        kw = dict(iter_first=1, max_iters=4, target_db=30.0, group_iters=2)
        kw.update(bad)
        with pytest.raises(capi.PtError, match="pt_render_until"):
            r.render_until(**kw)
        st = r.stats()
        assert st.device_bytes == before and st.samples == 0  # nothing allocated, nothing rendered
        assert r.noise() == dict(sse=-1.0, groups=0, iterations=0)
        assert not r.readback().any()
    finally:
        r.free()
