"""The variance-guided filter on the device (pt_denoise_guided, csrc/pt_denoise.hip) against the numpy restatement
tests/denoise_guided_ref.py, bit for bit.  The restatement is always fed with the GPU's own readbacks — image, feature buffers
and noise planes, each pinned by other tests — so these tests isolate the filter."""
import numpy as np
import pytest

import denoise_guided_ref as gref
import denoise_ref as ref
from denoise_ref import bits, f32

pytestmark = pytest.mark.gpu
RES = (97, 61)
SIZES = [2, 2, 2, 2]  # four groups of two iterations
M, T = len(SIZES), sum(SIZES)
OFF = dict(sigma_color=-1.0, sigma_normal=-1.0, sigma_position=-1.0)
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


def render_groups(r, sizes=SIZES, first=1):
    for n in sizes:
        r.render(first, n)
        r.noise_fold()
        first += n


def readbacks(r):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    return r.readback(), pack_planes(r.readback_features()), capi.join_noise(r.readback_noise())


def gpu_case(path, res, option_sets, **kw):
    """SIZES rendered with a fold after each group and T feature iterations, anti-aliased, then one guided call per option set:
    (image SUM, feature planes, noise planes, outputs)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    key = (path, tuple(res), repr(option_sets), tuple(sorted(kw.items())))
    if key not in _CASES:
        r = capi.Renderer(capi.Scene(path, res=res), aa_jitter=True, **kw)
        try:
            render_groups(r)
            r.render_features(1, T)
            _CASES[key] = readbacks(r) + ([r.denoise_guided(**o) for o in option_sets],)
        finally:
            r.free()
    return _CASES[key]


WHOLE = [dict(levels=1), dict(levels=3), dict(levels=5), dict(levels=5, keep_albedo=True)]


@pytest.mark.parametrize("k", range(len(WHOLE)))
def test_whole_frame_equals_restatement(scene_dir, k):
    img, planes, noise, outs = gpu_case(scene_dir["cornell"], RES, WHOLE)
    hits, var = planes[1, :, 3], noise[0, :, 3]
    assert (hits > 0).any() and (hits == 0).any() and int(((hits > 0) & (hits < T)).sum()) >= 100  # edges with fractional coverage
    assert (var == 0).any() and (var > 0).sum() >= 1000  # misses and emitters beside noisy pixels
    assert np.array_equal(bits(noise[0, :, :3]), bits(img))  # nothing rendered since the last fold
    stats = {}
    same(outs[k], gref.denoise_guided(img, planes, noise, RES[0], RES[1], M, T, stats=stats, **WHOLE[k]), WHOLE[k])
    assert stats["cut"] > 0


def test_it_is_not_the_unguided_filter(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    img, planes, noise, outs = gpu_case(scene_dir["cornell"], RES, WHOLE)
    differ = int((bits(outs[2]) != bits(capi.denoise_host(img, planes, RES[0], RES[1], T, levels=5))).any(axis=1).sum())
    print("pixels that differ between the guided and the unguided filter:", differ)
    assert differ >= 1000


@pytest.mark.parametrize("arith", ["fma", "fast"])
def test_modes_equal_restatement_of_their_own_readback(scene_dir, arith):
    img, planes, noise, outs = gpu_case(scene_dir["cornell"], RES, [dict()], arith=arith)
    same(outs[0], gref.denoise_guided(img, planes, noise, RES[0], RES[1], M, T), arith)


def test_contiguous_rows_tile(scene_dir):
    img, planes, noise, outs = gpu_case(scene_dir["cornell"], RES, [dict()], pixel_begin=97 * 7, pixel_count=97 * 20)
    assert outs[0].shape == (97 * 20, 3)
    same(outs[0], gref.denoise_guided(img, planes, noise, 97, 20, M, T), "rows 7 .. 26 as an image of their own")


def test_frame_smaller_than_a_workgroup_and_the_stencil(scene_dir):
    res = (33, 9)
    img, planes, noise, outs = gpu_case(scene_dir["cornell"], res, [dict(levels=5)])
    assert (planes[1, :, 3] > 0).any() and (planes[1, :, 3] == 0).any()
    same(outs[0], gref.denoise_guided(img, planes, noise, res[0], res[1], M, T, levels=5), res)


@pytest.mark.parametrize("w,rows", ref.FRAMES[:3])
def test_stage_equals_host(scene_dir, w, rows):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    groups, iters = 3, 7
    _, planes = ref.random_frame(w, rows, iters)
    noise = gref.random_noise_planes(w, rows, groups, iters)
    rgb = np.ascontiguousarray(noise[0, :, :3])
    if w * rows > 1:
        nonpositive, zero_variance, decades = gref.noise_properties(noise, groups, iters)
        assert nonpositive > 0 and zero_variance > 0 and decades >= 6.0
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(32, 24)))
    try:
        for opts in (dict(), dict(levels=8), dict(levels=3, keep_albedo=True), dict(levels=2, sigma_color=-1.0), dict(levels=2, sigma_color=3.0, sigma_normal=-1.0)):
            same(r.stage_denoise_guided(rgb, planes, noise, w, rows, groups, iters, **opts),
                 capi.denoise_guided_host(rgb, planes, noise, w, rows, groups, iters, **opts), (w, rows, opts))
        with pytest.raises(capi.PtError, match="pt_stage_denoise_guided.*at least 2"):
            r.stage_denoise_guided(rgb, planes, noise, w, rows, 1, iters)
    finally:
        r.free()


def test_group_equals_single_context(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    path, res = scene_dir["cornell"], (96, 60)
    _, _, _, outs = gpu_case(path, res, [dict(), dict(levels=3, keep_albedo=True)])
    L = capi.lib()
    g = capi.Group(capi.Scene(path, res=res), [0, 0, 0], transport="copy", aa_jitter=True)
    try:
        assert g.transport == "copy"
        g.render_features(1, T)
        with pytest.raises(capi.PtError, match="nothing has been folded"):
            g.denoise_guided()
        g.render(1, 2)
        g.noise_fold()
        with pytest.raises(capi.PtError, match="at least 2"):
            g.denoise_guided()
        render_groups(g, SIZES[1:], first=3)
        got = [g.denoise_guided(), g.denoise_guided(levels=3, keep_albedo=True)]
        with pytest.raises(capi.PtError, match="levels"):
            g.denoise_guided(levels=9)
        g.render(T + 1, 1)
        with pytest.raises(capi.PtError, match="fold first"):
            g.denoise_guided()
        g.noise_fold()
        one = L.pt_group_context(g._h, 1)  # one context a group ahead of the others
        capi._check(L.pt_ctx_render(one, T + 2, 1))
        capi._check(L.pt_ctx_noise_fold(one))
        with pytest.raises(capi.PtError, match="share"):
            g.denoise_guided()
    finally:
        g.free()
    same(got[0], outs[0], "three contexts on one device")
    same(got[1], outs[1], "three contexts on one device, 3 levels, keep_albedo")


def test_nothing_else_moves_and_the_unguided_result_stays(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = RES[0] * RES[1]
    for guided_first in (True, False):
        r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=RES), aa_jitter=True)
        try:
            render_groups(r)
            r.render_features(1, T)
            img, feats, noise = readbacks(r)
            before, est = r.stats(), r.noise()
            if not guided_first:
                unguided = r.denoise(T)
            first = r.denoise_guided()
            after = r.stats()
            assert after.device_bytes == before.device_bytes + 80 * n and after.samples == before.samples == T * n
            if guided_first:
                unguided = r.denoise(T)
            again = r.denoise_guided(levels=2)
            assert r.stats().device_bytes == after.device_bytes  # one workspace, whichever kind came first
            assert (bits(again) != bits(first)).any()
            same(r.denoise(T), unguided, "pt_denoise after pt_denoise_guided")
            same(r.denoise_guided(), first, "pt_denoise_guided after pt_denoise")
            now = readbacks(r)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(now, (img, feats, noise)))
            assert r.noise() == est and r.stats().samples == before.samples
        finally:
            r.free()
    _, _, _, outs = gpu_case(scene_dir["cornell"], RES, WHOLE)
    same(first, outs[2], "the shared case")


def test_errors(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    sc = capi.Scene(scene_dir["cornell"], res=RES)
    r = capi.Renderer(sc, pixel_begin=97 * 7, pixel_count=97 * 20, stripe_pixels=97, stripe_stride=194)
    try:
        render_groups(r, [1, 1])
        r.render_features(1, 2)
        before = r.stats().device_bytes
        with pytest.raises(capi.PtError, match="whole contiguous"):
            r.denoise_guided()
        assert r.stats().device_bytes == before
    finally:
        r.free()
    r = capi.Renderer(sc)
    try:
        r.render(1, 1)
        with pytest.raises(capi.PtError, match="no feature pass"):
            r.denoise_guided()
        r.render_features(1, 1)
        before = r.stats().device_bytes
        with pytest.raises(capi.PtError, match="nothing has been folded"):
            r.denoise_guided()
        assert r.stats().device_bytes == before
        r.noise_fold()
        before = r.stats().device_bytes
        with pytest.raises(capi.PtError, match="at least 2"):
            r.denoise_guided()
        r.render(2, 1)
        r.noise_fold()
        r.render(3, 1)
        with pytest.raises(capi.PtError, match="fold first"):
            r.denoise_guided()
        r.noise_fold()
        for bad, match in ((dict(levels=9), "levels"), (dict(sigma_normal=float("nan")), "sigma")):
            with pytest.raises(capi.PtError, match=match):
                r.denoise_guided(**bad)
        assert r.stats().device_bytes == before  # a refused call allocates nothing
        assert r.denoise_guided().shape == (RES[0] * RES[1], 3)
    finally:
        r.free()
