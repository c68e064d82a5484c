"""The variance-guided filter on the host (pt_denoise_guided_host: csrc/pt_denoise.h, the bodies the HIP kernels run too) against
the numpy restatement tests/denoise_guided_ref.py, bit for bit, and what it is for: a lower error than pt_denoise.  No GPU."""
import os

import numpy as np
import pytest

import denoise_guided_ref as gref
import denoise_ref as ref
import noise_ref
from denoise_ref import FRAMES, bits, f32

GROUPS, ITERS = 3, 7  # groups of 2, 2 and 3 iterations
OFF = dict(sigma_color=-1.0, sigma_normal=-1.0, sigma_position=-1.0)
OPTIONS = {
    "defaults": dict(),
    "keep_albedo": dict(keep_albedo=True),
    "own_sigmas": dict(sigma_color=3.0, sigma_normal=0.25, sigma_position=3.0),
    "colour_off": dict(sigma_color=-1.0),
}
_FRAMES = {}


def frame(w, rows):
    """(SUM image, feature SUM planes, noise planes) of a frame no renderer would produce; shared, read-only."""
    if (w, rows) not in _FRAMES:
        _, planes = ref.random_frame(w, rows, ITERS)
        noise = gref.random_noise_planes(w, rows, GROUPS, ITERS)
        rgb = np.ascontiguousarray(noise[0, :, :3])  # the image of the last fold: nothing was rendered since
        for a in (rgb, planes, noise):
            a.setflags(write=False)
        _FRAMES[(w, rows)] = (rgb, planes, noise)
    return _FRAMES[(w, rows)]


def same(got, want, what):
    got, want = np.asarray(got).reshape(len(want), -1), np.asarray(want).reshape(len(want), -1)
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:2]], want[bad[:2]])


@pytest.mark.parametrize("w,rows", FRAMES)
def test_random_planes_have_what_the_filter_branches_on(w, rows):
    rgb, planes, noise = frame(w, rows)
    nonpositive, zero_variance, decades = gref.noise_properties(noise, GROUPS, ITERS)
    print("d <= 0 components", nonpositive, "pixels of variance 0", zero_variance, "decades of variance", decades)
    assert noise.shape == (2, w * rows, 4) and not noise[1, :, 3].any()
    if w * rows == 1:
        return  # one pixel has one variance; the three larger frames carry the conditions
    assert nonpositive > 0 and zero_variance > 0 and decades >= 6.0, (nonpositive, zero_variance, decades)
    hits, misses, zero_albedo = ref.frame_properties(rgb, planes)
    assert hits > 0 and misses > 0 and zero_albedo > 0
    stats = {}
    gref.denoise_guided(rgb, planes, noise, w, rows, GROUPS, ITERS, levels=3, stats=stats)
    assert stats["cut"] > 0  # taps below exp32's cut-off
    assert (stats["var_0"] != stats["var_raw"]).any() and (stats["var"] != stats["var_0"]).any()


@pytest.mark.parametrize("name", sorted(OPTIONS))
@pytest.mark.parametrize("levels", [1, 3, 5, 8])
@pytest.mark.parametrize("w,rows", FRAMES)
def test_host_equals_restatement(w, rows, levels, name):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rgb, planes, noise = frame(w, rows)
    got = capi.denoise_guided_host(rgb, planes, noise, w, rows, GROUPS, ITERS, levels=levels, **OPTIONS[name])
    want = gref.denoise_guided(rgb, planes, noise, w, rows, GROUPS, ITERS, levels=levels, **OPTIONS[name])
    assert np.isfinite(want).all()
    same(got, want, (w, rows, levels, name))


@pytest.mark.parametrize("keep_albedo", [False, True])
@pytest.mark.parametrize("w,rows", FRAMES)
def test_variances_equal_restatement(w, rows, keep_albedo):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rgb, planes, noise = frame(w, rows)
    stats = {}
    gref.denoise_guided(rgb, planes, noise, w, rows, GROUPS, ITERS, levels=1, keep_albedo=keep_albedo, stats=stats)
    raw, pre = capi.denoise_guided_variance_host(rgb, planes, noise, w, rows, GROUPS, ITERS, keep_albedo=keep_albedo)
    same(raw, stats["var_raw"], "var_raw")
    same(pre, stats["var_0"], "var_0")


@pytest.mark.parametrize("levels", [1, 5])
@pytest.mark.parametrize("w,rows", FRAMES)
def test_colour_term_off_is_the_unguided_filter(w, rows, levels):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rgb, planes, noise = frame(w, rows)
    for opts in (dict(sigma_color=-1.0), dict(sigma_color=-1.0, keep_albedo=True), OFF):
        got = capi.denoise_guided_host(rgb, planes, noise, w, rows, GROUPS, ITERS, levels=levels, **opts)
        same(got, capi.denoise_host(rgb, planes, w, rows, ITERS, levels=levels, **opts), (w, rows, levels, opts))
    assert w * rows == 1 or (bits(capi.denoise_guided_host(rgb, planes, noise, w, rows, GROUPS, ITERS, levels=levels)) != bits(got)).any()


@pytest.mark.parametrize("npix", [1, 65, 1025])
@pytest.mark.parametrize("sizes", noise_ref.SEQUENCES[:3])
def test_prepared_variance_is_the_folds_own(npix, sizes):
    """(v_x + v_y) + v_z of the prepare step, without demodulation, equals the w plane the fold left, bit for bit (through the
    exposed helper pt_denoise_guided_variance_host: a level's (w * c) / w does not give c back to the bit)."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    sums, _ = noise_ref.random_sums(npix, sizes, 31 * npix + len(sizes))
    noise, T = noise_ref.new_planes(npix), 0
    for M, (n, S) in enumerate(zip(sizes, sums), start=1):
        T += n
        capi.noise_fold_host(S, noise, n, M, T)
    planes = np.zeros((3, npix, 4), f32)  # all misses: nothing to demodulate by either way
    raw, _ = capi.denoise_guided_variance_host(sums[-1], planes, noise, npix, 1, len(sizes), T, keep_albedo=True)
    assert (noise[0, :, 3] > 0).any() or npix == 1
    same(raw, noise[0, :, 3], (npix, sizes))


@pytest.mark.parametrize("bad,match", [
    (dict(levels=9), "levels"), (dict(levels=-1), "levels"), (dict(sigma_color=float("nan")), "sigma"), (dict(sigma_normal=float("inf")), "sigma"),
    (dict(sigma_position=float("-inf")), "sigma"), (dict(groups=1), "at least 2"), (dict(groups=0), "at least 2"), (dict(groups=3, iters=2), "iterations"),
])
def test_refusals(bad, match):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rgb, planes, noise = frame(5, 3)
    kw = dict(bad)
    groups, iters = kw.pop("groups", GROUPS), kw.pop("iters", ITERS)
    with pytest.raises(capi.PtError, match="pt_denoise_guided_host.*" + match):
        capi.denoise_guided_host(rgb, planes, noise, 5, 3, groups, iters, **kw)


def test_array_sizes_are_checked():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rgb, planes, noise = frame(5, 3)
    with pytest.raises(capi.PtError):
        capi.denoise_guided_host(rgb, planes, noise, 5, 4, GROUPS, ITERS)
    with pytest.raises(capi.PtError):
        capi.denoise_guided_host(rgb, planes, noise[:1], 5, 3, GROUPS, ITERS)


def test_sigma_color_zero_is_eight():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rgb, planes, noise = frame(33, 9)
    default = capi.denoise_guided_host(rgb, planes, noise, 33, 9, GROUPS, ITERS)
    same(capi.denoise_guided_host(rgb, planes, noise, 33, 9, GROUPS, ITERS, sigma_color=8.0, levels=5), default, "8")
    assert (bits(capi.denoise_guided_host(rgb, planes, noise, 33, 9, GROUPS, ITERS, sigma_color=4.0)) != bits(default)).any()


# ---- what it is for -------------------------------------------------------------------------------------------------------
RES = (97, 61)
_ORACLE = {}


def pack_planes(f):
    n = f["hits"].shape[0]
    planes = np.zeros((3, n, 4), f32)
    planes[0, :, :3], planes[0, :, 3] = f["normal"], f["depth"]
    planes[1, :, :3], planes[1, :, 3] = f["albedo"], f["hits"]
    planes[2, :, :3], planes[2, :, 3] = f["position"], f["object_id"].view(f32)
    return planes


def oracle_ratio(oracle, path, sizes, spp_truth=1024):
    """(raw, unguided, guided) error of the oracle's image of `path` at RES with anti-aliasing, rendered in groups of `sizes`
    iterations with a host fold after each; mean((min(x, 1) - min(truth, 1))^2), truth = spp_truth spp of other iterations."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    import features_ref
    threads = min(os.cpu_count() or 1, 16)
    n = RES[0] * RES[1]
    oracle.set_math_mode(oracle.PORTABLE)
    oracle.set_aa_jitter(True)
    try:
        oracle.load_scene(path, res=RES)
        if path not in _ORACLE:
            _ORACLE[path] = oracle.render(100001, spp_truth, variant=oracle.RETIRE, nthreads=threads).astype(np.float64) / spp_truth
        truth = _ORACLE[path]
        S, noise, T = None, noise_ref.new_planes(n), 0
        for M, k in enumerate(sizes, start=1):
            S = oracle.render(T + 1, k, variant=oracle.RETIRE, nthreads=threads, accum=S)
            T += k
            capi.noise_fold_host(S, noise, k, M, T)
    finally:
        oracle.set_aa_jitter(False)
    planes = pack_planes(features_ref.reference(oracle, path, RES, True, 1, T))

    def mse(x):
        return float(np.mean((np.minimum(x, 1).astype(np.float64) - np.minimum(truth, 1)) ** 2))
    return (mse(S / f32(T)), mse(capi.denoise_host(S, planes, RES[0], RES[1], T)),
            mse(capi.denoise_guided_host(S, planes, noise, RES[0], RES[1], len(sizes), T)))


def test_it_beats_the_unguided_filter(scene_dir, oracle):
    """cornell 97 x 61 with anti-aliasing against 1024 spp of other iterations, both filters at their defaults: the guided error
    is at most 0.85 of pt_denoise's at 4 groups of 4 iterations and at most 1.05 of it at 4 groups of 1.  (A numpy prototype of
    the specification measured 0.73 and 0.96.)  The sphere scene, which pt_denoise does not improve and whose noise is
    heavy-tailed, is printed and not asserted on."""
    results = {}
    for name, path, sizes in (("cornell 4 x 4", scene_dir["cornell"], [4] * 4), ("cornell 4 x 1", scene_dir["cornell"], [1] * 4),
                              ("sphere 4 x 4", scene_dir["sphere"], [4] * 4)):
        raw, unguided, guided = oracle_ratio(oracle, path, sizes)
        results[name] = guided / unguided
        print(f"{name}: raw {raw:.6g} unguided {unguided:.6g} guided {guided:.6g}  guided / unguided {guided / unguided:.4f}  unguided / raw {unguided / raw:.4f}")
    assert results["cornell 4 x 4"] <= 0.85, results
    assert results["cornell 4 x 1"] <= 1.05, results
