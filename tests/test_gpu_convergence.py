"""The convergence metric on the device (PtOptions.convergence, include/pt_amd.h): one SSE per iteration against a reference
frame, taken inside the gather kernel.

The judge is the numpy restatement of computePSNR's terms (pathtrace.cu:184-201) below, applied to per-iteration SUM images
of a SECOND renderer with the metric off — one pt_render(i, 1) and one readback per iteration (that batching changes no bit
of the image is pinned by tests/test_gpu_render.py).  The terms are float32 and bit-equal by construction, so GPU and judge
differ only in the order of a double sum: n * 2^-53 for n = 72,000 terms is 8e-12, and the bound of 1e-9 (relative) leaves
two orders of magnitude for any tree shape."""
import math
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "pt_render")
FLT_MAX = float(np.finfo(np.float32).max)
RES, ITERS, REL = (200, 120), 64, 1e-9
TILE = dict(pixel_begin=97 * 7, pixel_count=97 * 20, stripe_pixels=97, stripe_stride=97 * 2)  # tests/test_aa_extension.py's tile


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sse_restated(sum_image, iteration, ref):
    """cur = S / float(i) (a correctly rounded float32 division), d = cur - R, d.x*d.x + d.y*d.y + d.z*d.z left to right in
    float32 without FMA, summed over the pixels in double."""
    cur = sum_image / np.float32(iteration)
    d = cur - ref
    assert cur.dtype == np.float32 and d.dtype == np.float32
    term = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert term.dtype == np.float32
    return math.fsum(term.astype(np.float64).tolist())


_sums = {}


def sum_images(scene_path, res, iters, **kw):
    """SUM image after every iteration 1 .. iters from a renderer with the metric OFF: [iters][n, 3]."""
    key = (scene_path, res, iters, tuple(sorted(kw.items())))
    if key not in _sums:
        from cosc_4397_pathtracing_raytracing_project_amd import capi
        r = capi.Renderer(capi.Scene(scene_path, res=res), **kw)
        try:
            out = []
            for i in range(1, iters + 1):
                r.render(i, 1)
                out.append(r.readback())
        finally:
            r.free()
        _sums[key] = out
    return _sums[key]


def metric_run(scene_path, res, iters, **kw):
    """(curve [iters], final SUM image, PtStats) of one render of iterations 1 .. iters."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    ref = kw.pop("reference", None)
    r = capi.Renderer(capi.Scene(scene_path, res=res), **kw)
    try:
        if ref is not None:
            r.set_reference(ref)
        r.render(1, iters)
        return r.convergence(1, iters), r.readback(), r.stats(), r.iterations_to_clean(35.0)
    finally:
        r.free()


def check_curve(curve, sums, ref, first, label):
    """curve[i - 1] for i >= first against the restatement; prints every figure before asserting."""
    worst = 0.0
    for i in range(first, len(sums) + 1):
        want = sse_restated(sums[i - 1], i, ref)
        got = float(curve[i - 1])
        rel = abs(got - want) / want if want > 0 else abs(got)
        worst = max(worst, rel)
        print(f"{label}: iteration {i}: sse {got!r} restated {want!r} rel {rel:.3e}")
    print(f"{label}: worst relative difference {worst:.3e}")
    for i in range(first, len(sums) + 1):
        want = sse_restated(sums[i - 1], i, ref)
        got = float(curve[i - 1])
        assert got >= 0.0 and abs(got - want) <= REL * want, (label, i, got, want)


@pytest.mark.parametrize("kw", [
    {},
    dict(iters_per_batch=3),
    dict(iters_per_batch=7),  # iteration 10 inside a batch (8 .. 14); with 3 it opens one (10 .. 12), by default it is mid-batch
    dict(iters_per_batch=5),  # ... and iteration 10 as the last of its batch (6 .. 10)
    dict(unfused_bounces=True),
    dict(TILE),
    dict(num_queues=1, iters_per_batch=7),  # one queue owns all 24,000 pixels: the gather takes three passes, whose sums add up
], ids=["default", "batch3", "batch7", "batch5", "unfused_bounces", "striped_tile", "three_passes"])
def test_captured_reference_matches_restatement(scene_dir, kw):
    res = (97, 61) if "stripe_pixels" in kw else RES
    n = 10
    sums = sum_images(scene_dir["cornell"], res, ITERS, **{k: v for k, v in kw.items() if k in TILE})
    ref = sums[n - 1] / np.float32(n)
    curve, img, st, clean = metric_run(scene_dir["cornell"], res, ITERS, convergence=n, **kw)
    assert (curve[:n] == -1.0).all(), curve[:n]
    check_curve(curve, sums, ref, n + 1, f"captured {kw}")
    assert np.array_equal(bits(img), bits(sums[-1]))
    # two runs with equal options: bit-equal doubles; and off means off: the same image
    curve2, img2, _, clean2 = metric_run(scene_dir["cornell"], res, ITERS, convergence=n, **kw)
    assert np.array_equal(curve.view(np.uint64), curve2.view(np.uint64)) and clean == clean2
    _, img_off, st_off, _ = metric_run_off(scene_dir["cornell"], res, ITERS, **kw)
    assert np.array_equal(bits(img_off), bits(img))
    # the memory the metric adds: the formula of include/pt_amd.h
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    pixels = kw.get("pixel_count", res[0] * res[1])
    extra = 12 * pixels + 8 * st.iters_per_batch * st.num_queues * capi.CONVERGENCE_WAVES + 8 * capi.CONVERGENCE_CAPACITY
    assert (st.iters_per_batch, st.num_queues) == (st_off.iters_per_batch, st_off.num_queues)
    assert st.device_bytes - st_off.device_bytes == extra, (st.device_bytes, st_off.device_bytes, extra)
    # the README's "iterations to clean": the first iteration with a PSNR above 35 dB
    psnr = [capi.psnr_from_sse(float(s), pixels) if s >= 0 else None for s in curve]
    assert clean == next((i + 1 for i, p in enumerate(psnr) if p is not None and p > 35.0), -1)


def metric_run_off(scene_path, res, iters, **kw):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_path, res=res), convergence=0, **kw)
    try:
        r.render(1, iters)
        with pytest.raises(capi.PtError, match="convergence = 0"):
            r.convergence(1, iters)
        return None, r.readback(), r.stats(), None
    finally:
        r.free()


def test_supplied_reference_and_iterations_to_clean(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    sums = sum_images(scene_dir["cornell"], RES, ITERS)
    ref = sums[-1] / np.float32(ITERS)
    pixels = RES[0] * RES[1]
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=RES), convergence=-1)
    try:
        with pytest.raises(capi.PtError, match="no reference frame"):
            r.render(1, 1)
    finally:
        r.free()
    curve, img, _, clean = metric_run(scene_dir["cornell"], RES, ITERS, convergence=-1, reference=ref)
    check_curve(curve[:ITERS - 1], sums[:ITERS - 1], ref, 1, "supplied")
    assert curve[ITERS - 1] == 0.0 and capi.psnr_from_sse(float(curve[ITERS - 1]), pixels) == FLT_MAX
    assert np.array_equal(bits(img), bits(sums[-1]))
    # iterations to clean at 35 dB against the restatement's own curve
    want_psnr = [capi.psnr_from_sse(sse_restated(sums[i - 1], i, ref), pixels) for i in range(1, ITERS + 1)]
    for i, p in enumerate(want_psnr):
        print(f"supplied: iteration {i + 1}: restated psnr {p:.4f} dB")
    near = [(i + 1, p) for i, p in enumerate(want_psnr) if abs(p - 35.0) < 0.01]
    assert not near, f"a PSNR within 0.01 dB of the threshold makes the answer depend on rounding: {near}"
    want_clean = next((i + 1 for i, p in enumerate(want_psnr) if p > 35.0), -1)
    print(f"supplied: iterations to clean {clean}, restated {want_clean}")
    assert clean == want_clean
    assert want_clean == 39  # the CPU oracle's answer (PORTABLE mode, which the exact kernels equal bit for bit)


@pytest.mark.parametrize("arith", ["fma", "fast"])
def test_modes_match_the_restatement_on_their_own_images(scene_dir, arith):
    n = 10
    sums = sum_images(scene_dir["cornell"], RES, ITERS, arith=arith)
    ref = sums[n - 1] / np.float32(n)
    curve, img, _, _ = metric_run(scene_dir["cornell"], RES, ITERS, convergence=n, arith=arith)
    assert (curve[:n] == -1.0).all()
    check_curve(curve, sums, ref, n + 1, arith)
    assert np.array_equal(bits(img), bits(sums[-1]))


def test_group_of_three_contexts_adds_up_to_the_single_context_curve(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = 10
    single, img1, _, clean1 = metric_run(scene_dir["cornell"], RES, ITERS, convergence=n)
    g = capi.Group(capi.Scene(scene_dir["cornell"], res=RES), [0, 0, 0], convergence=n)
    try:
        assert g.transport == "copy"
        g.render(1, ITERS)
        curve = g.convergence(1, ITERS)
        clean = g.iterations_to_clean(35.0)
        img = g.gather()
    finally:
        g.free()
    assert np.array_equal(bits(img), bits(img1))
    assert (curve[:n] == -1.0).all()
    for i in range(n + 1, ITERS + 1):
        print(f"group: iteration {i}: {curve[i - 1]!r} single {single[i - 1]!r}")
        assert abs(curve[i - 1] - single[i - 1]) <= REL * single[i - 1], i
    assert clean == clean1 and clean > n
    # ... and with a supplied W*H frame, of which every context takes its rows
    sums = sum_images(scene_dir["cornell"], RES, ITERS)
    ref = sums[-1] / np.float32(ITERS)
    single, _, _, clean1 = metric_run(scene_dir["cornell"], RES, ITERS, convergence=-1, reference=ref)
    g = capi.Group(capi.Scene(scene_dir["cornell"], res=RES), [0, 0, 0], convergence=-1)
    try:
        g.set_reference(ref)
        g.render(1, ITERS)
        curve = g.convergence(1, ITERS)
        clean = g.iterations_to_clean(35.0)
    finally:
        g.free()
    assert curve[-1] == 0.0
    assert (np.abs(curve - single) <= REL * single).all()
    assert clean == clean1 == 39


def test_large_table_scene(scene_dir):
    res, iters, n = (160, 90), 12, 4
    sums = sum_images(scene_dir["stress_big"], res, iters)
    curve, img, _, _ = metric_run(scene_dir["stress_big"], res, iters, convergence=n)
    assert (curve[:n] == -1.0).all()
    check_curve(curve, sums, sums[n - 1] / np.float32(n), n + 1, "stress_big")
    assert np.array_equal(bits(img), bits(sums[-1]))


def test_queues_without_pixels_contribute_nothing(scene_dir):
    res, iters, n = (100, 7), 12, 4  # 11 chunks of 64 pixels for 256 queues, the last one partial
    sums = sum_images(scene_dir["cornell"], res, iters)
    curve, img, _, _ = metric_run(scene_dir["cornell"], res, iters, convergence=n, num_queues=256, iters_per_batch=5)
    assert (curve[:n] == -1.0).all()
    check_curve(curve, sums, sums[n - 1] / np.float32(n), n + 1, "100x7")
    assert np.array_equal(bits(img), bits(sums[-1]))


def test_clear_rearms_the_capture_and_forgets_the_curve(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=RES), convergence=10, iters_per_batch=7)
    try:
        r.render(1, ITERS)
        first = r.convergence(1, ITERS + 4)
        assert (first[ITERS:] == -1.0).all() and (r.convergence(-2, 3) == -1.0).all()  # never rendered / outside 1 .. capacity
        r.clear()
        assert (r.convergence(1, ITERS) == -1.0).all() and r.iterations_to_clean(35.0) == -1
        r.render(1, 20)
        r.render(21, ITERS - 20)
        second = r.convergence(1, ITERS + 4)
        with pytest.raises(capi.PtError, match="PT_CONVERGENCE_CAPACITY"):
            r.render(capi.CONVERGENCE_CAPACITY, 2)
        with pytest.raises(capi.PtError, match="not -1"):
            r.set_reference(np.zeros((RES[0] * RES[1], 3), np.float32))
    finally:
        r.free()
    assert np.array_equal(first.view(np.uint64), second.view(np.uint64))
    for bad in (-2, capi.CONVERGENCE_CAPACITY + 1):
        with pytest.raises(capi.PtError, match="convergence"):
            capi.Renderer(capi.Scene(scene_dir["cornell"], res=RES), convergence=bad)


def test_shim_psnr_is_what_the_reference_prints(scene_dir, tmp_path):
    """`pt_render --convergence 10` goes through pathtraceSetConvergence / pathtrace / pathtracePSNR and prints one line per
    iteration: "Inf" up to the captured frame, then pt_psnr_from_sse of the captured-reference curve."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    curve, _, _, clean = metric_run(scene_dir["cornell"], RES, ITERS, convergence=10)
    r = subprocess.run([BIN, scene_dir["cornell"], "--res", f"{RES[0]}x{RES[1]}", "--spp", str(ITERS), "--depth", "8", "--convergence", "10",
                        "--out", str(tmp_path / "c")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [l.split() for l in r.stdout.splitlines() if l[:1].isdigit() and len(l.split()) == 2]
    assert [int(a) for a, _ in lines] == list(range(1, ITERS + 1))
    for (it, val), sse in zip(lines, curve):
        if int(it) <= 10:
            assert val == "Inf"
        else:
            assert np.float32(val) == np.float32(capi.psnr_from_sse(float(sse), RES[0] * RES[1])), (it, val)
    assert f"Iterations to clean: {clean}" in r.stdout
