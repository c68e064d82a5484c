"""The noise estimate on the host (pt_noise_fold_host: csrc/pt_noise.h, the body the HIP kernel runs too) against the numpy
restatement tests/noise_ref.py, bit for bit; and the estimator against the truth, with the oracle's images.  No GPU."""
import os

import numpy as np
import pytest

import noise_ref as ref
from noise_ref import PIXELS, SEQUENCES, bits, f32


@pytest.mark.parametrize("npix", PIXELS)
def test_random_sums_have_what_the_fold_branches_on(npix):
    sums, cls = ref.random_sums(npix, SEQUENCES[0], seed=npix)
    if npix < 63:
        return  # one pixel is of one class; the larger frames carry the conditions
    assert all((cls == k).any() for k in range(5))
    planes = ref.new_planes(npix)
    T, d_signs, denormal = 0, set(), False
    tiny = np.finfo(f32).tiny
    for M, (n, S) in enumerate(zip(SEQUENCES[0], sums), start=1):
        b = S - planes[0, :, :3]
        with np.errstate(under="ignore"):
            bb = b * b
        denormal |= bool(((bb > 0) & (bb < tiny)).any())
        T += n
        ref.fold(S, planes, n, M, T)
        if M >= 2:
            with np.errstate(under="ignore"):
                d = planes[1, :, :3] - (S * S) / f32(T)
            const = d[cls == 2]
            d_signs |= {int(s) for s in np.sign(const).ravel()}
            assert (planes[0, cls == 1, 3] == 0).all() and (planes[1, cls == 1] == 0).all()
    assert denormal, "no denormal product"
    assert {-1, 1} <= d_signs, d_signs  # constant pixels: the residue lands on either side of zero
    assert (planes[0, cls == 0, 3] > 0).all()


@pytest.mark.parametrize("groups", SEQUENCES)
@pytest.mark.parametrize("npix", PIXELS)
def test_host_equals_restatement(npix, groups):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    sums, _ = ref.random_sums(npix, groups, seed=1000 + npix)
    got, want = ref.new_planes(npix), ref.new_planes(npix)
    T = 0
    for M, (n, S) in enumerate(zip(groups, sums), start=1):
        T += n
        sse = capi.noise_fold_host(S, got, n, M, T)
        w, want_sse = ref.fold(S, want, n, M, T)
        assert np.isfinite(want).all()
        bad = np.flatnonzero((bits(got) != bits(want)).reshape(2, npix, 4).any(axis=(0, 2)))
        assert bad.size == 0, (M, bad.size, bad[:8], got[:, bad[:2]], want[:, bad[:2]])
        if M < 2:
            assert sse == -1.0 and not bits(got[0, :, 3]).any()
        else:
            exact = float(np.sum(w.astype(np.float64)))
            assert sse >= 0 and abs(sse - exact) <= 1e-9 * exact, (M, sse, exact)
        assert not bits(got[1, :, 3]).any()  # +0
        assert np.array_equal(bits(got[0, :, :3]), bits(S))


def test_split_noise_names_the_planes():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    p = np.arange(2 * 5 * 4, dtype=f32).reshape(2, 5, 4)
    s = capi.split_noise(p)
    assert np.array_equal(s["prev"], p[0, :, :3]) and np.array_equal(s["q"], p[1, :, :3]) and np.array_equal(s["variance"], p[0, :, 3])


@pytest.mark.parametrize("bad", [dict(group_iters=0), dict(groups_after=0), dict(group_iters=4, groups_after=2, iters_after=4),
                                 dict(group_iters=-1)])
def test_bad_scalars_are_refused(bad):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    kw = dict(group_iters=1, groups_after=1, iters_after=1)
    kw.update(bad)
    planes = ref.new_planes(3)
    with pytest.raises(capi.PtError, match="pt_noise_fold_host"):
        capi.noise_fold_host(np.ones((3, 3), f32), planes, **kw)
    assert not planes.any()


def test_array_sizes_are_checked():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    with pytest.raises(capi.PtError):
        capi.noise_fold_host(np.ones((3, 3), f32), ref.new_planes(4), 1, 1, 1)
    with pytest.raises(capi.PtError):
        capi.noise_fold_host(np.ones((3, 3), f32), np.zeros((2, 3, 4), np.float64), 1, 1, 1)


def test_the_estimator_estimates(scene_dir, oracle):
    """cornell 64x48 with anti-aliasing, eight groups of four iterations, against 2048 spp of other iterations: at every
    M >= 2  SSE_est / sum (S / T - truth)^2  lies in [2/3, 3/2].  (The truth's own noise makes the expectation
    1 / (1 + T / 2048); measured 0.956 .. 1.023.  The sphere scene's heavy tails, 0.75 .. 2.04, are why it is not used.)"""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res, groups = (64, 48), [4] * 8
    threads = min(os.cpu_count() or 1, 16)
    oracle.set_math_mode(oracle.PORTABLE)
    oracle.set_aa_jitter(True)
    try:
        oracle.load_scene(scene_dir["cornell"], res=res)
        truth = oracle.render(100001, 2048, variant=oracle.RETIRE, nthreads=threads).astype(np.float64) / 2048
        S, planes, T = None, ref.new_planes(res[0] * res[1]), 0
        ratios = []
        for M, n in enumerate(groups, start=1):
            S = oracle.render(T + 1, n, variant=oracle.RETIRE, nthreads=threads, accum=S)
            T += n
            sse = capi.noise_fold_host(S, planes, n, M, T)
            if M >= 2:
                actual = float(np.sum((S.astype(np.float64) / T - truth) ** 2))
                ratios.append(sse / actual)
    finally:
        oracle.set_aa_jitter(False)
    print("SSE_est / actual at M = 2 ..:", [round(r, 4) for r in ratios])
    assert len(ratios) == 7 and all(2 / 3 <= r <= 3 / 2 for r in ratios), ratios
