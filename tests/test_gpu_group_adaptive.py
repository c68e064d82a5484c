"""Adaptive sampling by threshold across a group of contexts (pt_group_adaptive_round_threshold, pt_group_render_threshold and the
write-outs pt_group_gather_adaptive / _resolve / _denoise_adaptive; csrc/pt_group.cpp, csrc/pt_group_select.hip) and the round over
a caller's list it is built on (pt_adaptive_round_list; csrc/pt_post.cpp): a group holds, bit for bit, what ONE renderer holds after
the same calls.  Cornell at 97x61 (61 rows: the contexts own 31/30 and 21/20/20 of them), groups of 3 iterations."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref as ref
import adaptive_threshold_ref as tref
import group_select_ref as gref
from adaptive_ref import bits, f32

pytestmark = pytest.mark.gpu
G = 3
RES = (97, 61)
N = RES[0] * RES[1]
CAP_FRACTION = 0.25
MODES = [("exact", False), ("fast", True)]
MODE_IDS = ["exact-shared", "fast-jitter"]


def visible_devices():
    import torch
    return torch.cuda.device_count()


def raw_planes(r):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    out = np.empty((2, r.n, 4), f32)
    capi._check(capi.lib().pt_readback_noise(capi._f(out)))
    return out


def context_planes(g, i, rows):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    out = np.empty((2, rows * g.scene.resolution[0], 4), f32)
    capi._check(capi.lib().pt_ctx_readback_noise(g.context(i), capi._f(out)))
    return out


def warm_up(r, groups=2, n=G, first=1):
    for j in range(groups):
        r.render(first + j * n, n)
        r.noise_fold()


def threshold_for(planes, counts, want_above, res=RES):
    """A threshold that leaves about want_above pixels above (tests/test_gpu_adaptive_threshold.py)."""
    k = np.sort(ref.keys(planes[0, :, 3], res[0], res[1], counts).view(f32))[::-1]
    return float(np.sqrt(np.float64(k[want_above]))) * (1 + 1e-6)


def threshold_leaving(planes, counts, want, res=RES):
    """A threshold that leaves exactly `want` pixels above: the smallest float32 t whose square, in float32, is not below the key at
    rank `want`; the key one rank up must exceed that square."""
    k = np.sort(ref.keys(planes[0, :, 3], res[0], res[1], counts).view(f32))[::-1]
    t = f32(np.sqrt(np.float64(k[want])))
    while f32(t * t) < k[want]:
        t = np.nextafter(t, f32(np.inf))
    assert f32(t * t) < k[want - 1], (want, k[:want + 1])
    return float(t)


def same_bits(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero((bits(a) != bits(b)).reshape(a.shape[0], -1).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:8], a[bad[:2]], b[bad[:2]])


# ---- (a) the partition's kernels against the host function -------------------------------------------------------------------------
@pytest.mark.parametrize("w, h, n", gref.SHAPES)
def test_partition_kernels_equal_host(scene_dir, w, h, n):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(33, 9)))
    try:
        for name, lst in gref.cases(w, h, n):
            want_parts, want_counts = capi.group_partition_host(lst, w, h, n)
            parts, counts = capi.stage_group_partition(lst, w, h, n)
            assert np.array_equal(counts, want_counts), (w, h, n, name, counts, want_counts)
            for i in range(n):
                assert np.array_equal(parts[i], want_parts[i]), (w, h, n, name, i, parts[i][:8], want_parts[i][:8])
        with pytest.raises(capi.PtError, match=r"pt_stage_group_partition: .*list\[1\] = 2"):
            capi.stage_group_partition(np.array([3, 2], np.int32), w, h, n)
    finally:
        r.free()


# ---- (b) a round over a caller's list ------------------------------------------------------------------------------------------------
class OneContext:
    """A group of one context, driven like a Renderer; its rounds take the list from DEVICE memory."""

    def __init__(self, scene, **kw):
        from cosc_4397_pathtracing_raytracing_project_amd import capi
        self.g = capi.Group(scene, [0], **kw)
        self.n = scene.resolution[0] * scene.resolution[1]
        for name in ("render", "noise_fold", "noise", "resolve", "free"):
            setattr(self, name, getattr(self.g, name))
        self.readback, self.readback_adaptive, self.stats = self.g.gather, self.g.gather_adaptive, lambda: self.g.stats(0)

    def planes(self):
        return context_planes(self.g, 0, self.g.scene.resolution[1])

    def adaptive_round_list(self, iter_first, group_iters, lst, capacity):
        import torch
        from cosc_4397_pathtracing_raytracing_project_amd import capi
        self.keep = torch.tensor(np.asarray(lst, np.int32), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ptr = C.c_void_p(self.keep.data_ptr() if len(lst) else None)
        capi._check(capi.lib().pt_ctx_adaptive_round_list_device(self.g.context(0), int(iter_first), int(group_iters), ptr, len(lst), int(capacity)))


def state_of(r, planes):
    return dict(S=r.readback(), planes=planes, counts=r.readback_adaptive(), noise=r.noise(), samples=r.stats().samples, resolved=r.resolve())


ROUNDS = (None, 70, -1)  # pixels above: more than the cap (m == cap), a short list, none (m == 0)


@pytest.mark.parametrize("arith, aa_jitter", MODES, ids=MODE_IDS)
def test_round_list_equals_threshold_round(scene_dir, arith, aa_jitter):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(scene_dir["cornell"], res=RES)
    kw = dict(arith=arith, aa_jitter=aa_jitter, iters_per_batch=G)
    cap = ref.list_length(CAP_FRACTION, N)
    r = capi.Renderer(scene, **kw)
    try:
        warm_up(r)
        want, lists = [state_of(r, raw_planes(r))], []
        for k, want_above in enumerate(ROUNDS):
            planes, counts = want[-1]["planes"], want[-1]["counts"]
            threshold = 0.0 if want_above is None else 1e3 if want_above < 0 else threshold_for(planes, counts, want_above)
            lst, above, m = tref.select_threshold(planes[0, :, 3], RES[0], RES[1], counts, threshold, cap)
            assert r.adaptive_round_threshold(1 + (2 + k) * G, G, threshold, CAP_FRACTION) == (above, m)
            lists.append(np.asarray(lst, np.int32))
            want.append(state_of(r, raw_planes(r)))
        assert [l.size for l in lists] == [cap, lists[1].size, 0] and 0 < lists[1].size < cap
    finally:
        r.free()

    def follow(make, planes_of, what):
        r = make()
        try:
            warm_up(r)
            for k, lst in enumerate(lists):
                before = r.noise()
                r.adaptive_round_list(1 + (2 + k) * G, G, lst, cap)
                got, w = state_of(r, planes_of(r)), want[k + 1]
                for name in ("S", "resolved"):
                    same_bits(got[name], w[name], (what, k, name))
                same_bits(got["planes"].reshape(2 * N, 4), w["planes"].reshape(2 * N, 4), (what, k, "planes"))
                assert np.array_equal(got["counts"], w["counts"]) and got["samples"] == w["samples"], (what, k)
                if lst.size:
                    assert got["noise"] == w["noise"], (what, k, got["noise"], w["noise"])
                else:  # an empty list renders nothing and leaves SSE_est, and still counts the round and its iterations
                    assert got["noise"] == dict(sse=before["sse"], groups=before["groups"] + 1, iterations=(3 + k) * G), (what, got["noise"], before)
        finally:
            r.free()

    follow(lambda: capi.Renderer(scene, **kw), raw_planes, "host list")
    follow(lambda: OneContext(scene, **kw), lambda r: r.planes(), "device list")


@pytest.mark.parametrize("arith, aa_jitter", MODES, ids=MODE_IDS)
def test_round_list_on_a_striped_tile(scene_dir, arith, aa_jitter):
    """Rows 1 and 3 of a 33x9 frame as one striped tile (tests/test_gpu_refusals.py): the merged rows equal the same rows of a
    whole-frame renderer given the corresponding list."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    W, H = 33, 9
    scene = capi.Scene(scene_dir["cornell"], res=(W, H))
    kw = dict(arith=arith, aa_jitter=aa_jitter, iters_per_batch=G)
    rng = np.random.default_rng(3)
    tile_list = np.sort(rng.choice(2 * W, 23, replace=False)).astype(np.int32)  # both rows, the stripe's boundary included
    tile_list[[0, 11, 12, -1]] = (0, W - 1, W, 2 * W - 1)
    tile_list = np.unique(tile_list).astype(np.int32)
    frame_list = gref.frame_pixels(tile_list, 1, W, 2).astype(np.int32)  # the tile starts at row 1 and takes every second row
    rows = np.concatenate([np.arange(W, 2 * W), np.arange(3 * W, 4 * W)])
    assert set(frame_list) <= set(rows) and (frame_list >= 3 * W).any() and (frame_list < 2 * W).any()

    def run(lst, capacity, **tile):
        r = capi.Renderer(scene, **kw, **tile)
        try:
            warm_up(r)
            r.adaptive_round_list(1 + 2 * G, G, lst, capacity)
            r.adaptive_round_list(1 + 3 * G, G, lst[::3], capacity)  # the same worker at a shorter live length
            return r.readback(), raw_planes(r), r.readback_adaptive(), r.resolve(), r.stats().samples
        finally:
            r.free()

    whole = run(frame_list, 2 * W)
    striped = run(tile_list, 2 * W, pixel_begin=W, pixel_count=2 * W, stripe_pixels=W, stripe_stride=2 * W)
    assert (whole[2][frame_list, 1] >= 3).all() and whole[2][:, 1].max() == 4
    same_bits(striped[0], whole[0][rows], "image")
    same_bits(striped[1].reshape(-1, 4), whole[1][:, rows].reshape(-1, 4), "planes")
    assert np.array_equal(striped[2], whole[2][rows])
    same_bits(striped[3], whole[3][rows], "resolved")
    assert striped[4] - 2 * G * 2 * W == whole[4] - 2 * G * W * H == G * (tile_list.size + tile_list[::3].size)


def test_round_list_refuses(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    W, H = 33, 9
    scene = capi.Scene(scene_dir["cornell"], res=(W, H))
    r = capi.Renderer(scene, iters_per_batch=G)
    try:
        def refused(match, first, iters, lst, capacity):
            before = r.stats().device_bytes
            with pytest.raises(capi.PtError, match="pt_adaptive_round_list: .*" + match):
                r.adaptive_round_list(first, iters, np.array(lst, np.int32), capacity)
            assert r.stats().device_bytes == before, match

        refused("0 group", 1, G, [0, 1], 2)
        warm_up(r)
        r.render(1 + 2 * G, G)
        refused("fold first", 1 + 3 * G, G, [0, 1], 2)
        r.noise_fold()
        refused("at least one", 1 + 3 * G, 0, [0, 1], 2)
        refused("a list of 3 on a worker for 2", 1 + 3 * G, G, [0, 1, 2], 2)
        refused("a worker for 0", 1 + 3 * G, G, [], 0)
        refused(f"a worker for {W * H + 1}", 1 + 3 * G, G, [0], W * H + 1)
        refused(r"list\[2\] = 1 ", 1 + 3 * G, G, [0, 1, 1], 4)
        refused(r"list\[1\] = 0 ", 1 + 3 * G, G, [5, 0], 4)
        refused(rf"list\[0\] = {W * H} ", 1 + 3 * G, G, [W * H], 4)
        assert r.noise()["groups"] == 3 and np.array_equal(r.readback_adaptive(), ref.uniform_counts(W * H, 3 * G, 3))  # still the uniform state
    finally:
        r.free()
    r = capi.Renderer(scene, iters_per_batch=G, convergence=2)
    try:
        warm_up(r)
        with pytest.raises(capi.PtError, match="pt_adaptive_round_list: .*convergence"):
            r.adaptive_round_list(1 + 2 * G, G, np.array([0], np.int32), 1)
    finally:
        r.free()


# ---- (c) the group's round against one renderer making the same calls ------------------------------------------------------------------
def group_rounds(scene_dir, devices, arith, aa_jitter):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(scene_dir["cornell"], res=RES)
    kw = dict(arith=arith, aa_jitter=aa_jitter, iters_per_batch=G)
    n = len(devices)
    rows = [(RES[1] - i + n - 1) // n for i in range(n)]
    row_of = np.arange(N) // RES[0]
    cap = ref.list_length(CAP_FRACTION, N)
    r = capi.Renderer(scene, **kw)
    g = capi.Group(scene, devices, **kw)
    try:
        warm_up(r)
        warm_up(g)

        def context_samples():
            return [g.stats(i).samples for i in range(n)]

        def same_state(what):
            same_bits(g.gather(), r.readback(), (what, "image"))
            assert np.array_equal(g.gather_adaptive(), r.readback_adaptive()), (what, "counts")
            same_bits(g.resolve(), r.resolve(), (what, "resolved"))
            planes = raw_planes(r)
            for i in range(n):
                same_bits(context_planes(g, i, rows[i]).reshape(-1, 4), planes[:, row_of % n == i].reshape(-1, 4), (what, "planes of context", i))
            got, want = g.noise(), r.noise()
            assert (got["groups"], got["iterations"]) == (want["groups"], want["iterations"]), (what, got, want)
            assert abs(got["sse"] - want["sse"]) <= 1e-9 * want["sse"], (what, got, want)  # added per context, then in context order
            assert sum(context_samples()) == r.stats().samples, what

        same_state("uniform")
        assert np.array_equal(g.gather_adaptive(), ref.uniform_counts(N, 2 * G, 2))
        lengths = []
        # a list cut by the cap; lists that shrink to a handful of pixels and then to ONE; nothing above; and a cut list again
        for k, want_above in enumerate((None, cap // 2, cap // 8, 70, 3, 1, -1, None)):
            pick = threshold_leaving if want_above in (3, 1) else threshold_for
            threshold = 0.0 if want_above is None else 1e3 if want_above < 0 else pick(raw_planes(r), r.readback_adaptive(), want_above)
            what = (devices, arith, aa_jitter, k, want_above, threshold)
            before = context_samples()
            want = r.adaptive_round_threshold(1 + (2 + k) * G, G, threshold, CAP_FRACTION)
            got = g.adaptive_round_threshold(1 + (2 + k) * G, G, threshold, CAP_FRACTION)
            assert got == want, (what, got, want)
            above, m = got
            if want_above is None:
                assert above > cap == m, what
            elif want_above < 0:
                assert (above, m) == (0, 0) and context_samples() == before, what
            else:
                assert 0 < above == m < cap and (want_above > 3 or m == want_above), (what, above, m)
            if want_above == 1:  # one context renders the pixel, the others nothing, and all of them count the round
                grew = [a - b for a, b in zip(context_samples(), before)]
                assert sorted(grew) == [0] * (n - 1) + [G], (what, grew)
            lengths.append(m)
            same_state(what)
        assert lengths[0] == lengths[-1] == cap and lengths[5] == 1 and lengths[6] == 0
        # the filter that reads the counts; the two that do not still refuse the adaptive state
        r.render_features(1, 4)
        g.render_features(1, 4)
        same_bits(g.denoise_adaptive(), r.denoise_adaptive(), "denoise_adaptive")
        same_bits(g.denoise_adaptive(levels=3, keep_albedo=True), r.denoise_adaptive(levels=3, keep_albedo=True), "denoise_adaptive, 3 levels")
        for call, args in ((g.denoise, (4.0,)), (g.denoise_guided, ())):
            with pytest.raises(capi.PtError, match="adaptive state"):
                call(*args)
        same_state("after the filters")
    finally:
        g.free()
        r.free()


@pytest.mark.parametrize("contexts", [2, 3])
@pytest.mark.parametrize("arith, aa_jitter", MODES, ids=MODE_IDS)
def test_group_rounds_equal_single_context(scene_dir, contexts, arith, aa_jitter):
    group_rounds(scene_dir, [0] * contexts, arith, aa_jitter)


def test_group_rounds_on_every_visible_device(scene_dir):
    """The RCCL branch of both exchanges: the packed pairs to the root, the parts back."""
    ndev = visible_devices()
    if ndev < 2:
        pytest.skip("one visible device: the RCCL exchanges need two")
    group_rounds(scene_dir, list(range(ndev)), "exact", False)


def test_uniform_state_write_outs(scene_dir):
    """pt_group_denoise_adaptive, _resolve and _gather_adaptive before any round: the shared (T, M) for every pixel."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(scene_dir["cornell"], res=RES)
    kw = dict(aa_jitter=True, iters_per_batch=G)
    r = capi.Renderer(scene, **kw)
    g = capi.Group(scene, [0, 0, 0], **kw)
    try:
        for x in (r, g):
            x.render_features(1, 2)
        with pytest.raises(capi.PtError, match="pt_group_denoise_adaptive: nothing has been folded"):
            g.denoise_adaptive()
        for x in (r, g):
            x.render(1, G)
            x.noise_fold()
        with pytest.raises(capi.PtError, match=r"pt_group_denoise_adaptive: 1 group\(s\) folded"):
            g.denoise_adaptive()
        for x in (r, g):
            x.render(1 + G, G)
        with pytest.raises(capi.PtError, match="pt_group_denoise_adaptive: context 0 .*fold first"):
            g.denoise_adaptive()
        for x in (r, g):
            x.noise_fold()
        with pytest.raises(capi.PtError, match="pt_group_denoise_adaptive: .*levels"):
            g.denoise_adaptive(levels=9)
        same_bits(g.denoise_adaptive(), r.denoise_adaptive(), "uniform state")
        same_bits(g.resolve(), r.resolve(), "resolved")
        assert np.array_equal(g.gather_adaptive(), r.readback_adaptive()) and np.array_equal(g.gather_adaptive(), ref.uniform_counts(N, 2 * G, 2))
    finally:
        g.free()
        r.free()


# ---- (d) the driver ---------------------------------------------------------------------------------------------------------------------
def test_group_render_threshold_equals_single_context(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(scene_dir["cornell"], res=(96, 54))
    r = capi.Renderer(scene, arith="exact")
    g = capi.Group(scene, [0, 0], arith="exact")
    try:
        want = r.render_threshold(1, 40, 0.05, max_fraction=0.25, group_iters=4)
        got = g.render_threshold(1, 40, 0.05, max_fraction=0.25, group_iters=4)
        assert got == want and want[0] == 40 and want[1] < 40 * 96 * 54 and want[2] > 0, (got, want)
        same_bits(g.gather(), r.readback(), "image")
        same_bits(g.resolve(), r.resolve(), "resolved")
        assert np.array_equal(g.gather_adaptive(), r.readback_adaptive())
        assert g.stats(0).samples + g.stats(1).samples == r.stats().samples == want[1]
        assert (g.noise()["groups"], g.noise()["iterations"]) == (r.noise()["groups"], r.noise()["iterations"]) == (10, 40)
    finally:
        g.free()
        r.free()


# ---- (e) refusals ---------------------------------------------------------------------------------------------------------------------------
def test_group_refusals_allocate_nothing(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    L = capi.lib()
    res = (33, 9)

    def refused(g, match, *args, call="adaptive_round_threshold"):
        before = sum(g.stats(i).device_bytes for i in range(3))
        with pytest.raises(capi.PtError, match=f"pt_group_{call}: .*{match}"):
            getattr(g, call)(*args)
        assert sum(g.stats(i).device_bytes for i in range(3)) == before, match

    g = capi.Group(capi.Scene(scene_dir["cornell"], res=res), [0, 0, 0], iters_per_batch=G)
    try:
        refused(g, "0 group", 1, G, 0.1, 0.25)
        warm_up(g, groups=1)
        refused(g, "1 group", 1 + G, G, 0.1, 0.25)
        warm_up(g, groups=1, first=1 + G)
        g.render(1 + 2 * G, G)
        refused(g, "fold first", 1 + 3 * G, G, 0.1, 0.25)
        g.noise_fold()
        for threshold in (-0.1, float("nan"), float("inf")):
            refused(g, "threshold", 1 + 3 * G, G, threshold, 0.25)
            refused(g, "threshold", 1 + 3 * G, 10, threshold, 0.25, call="render_threshold")
        for fraction in (0.0, 1.5, float("nan")):
            refused(g, "fraction", 1 + 3 * G, G, float("nan"), fraction)  # the order of pt_adaptive_round's refusals first
        refused(g, "at least one", 1 + 3 * G, 0, 0.1, 0.25)
        refused(g, "pixels >= 0", 1 + 3 * G, 10, 0.1, 0.25, 0, -1, call="render_threshold")
        one = g.context(1)  # one context a group ahead of the others
        capi._check(L.pt_ctx_render(one, 1 + 3 * G, G))
        refused(g, "fold first", 1 + 4 * G, G, 0.1, 0.25)
        capi._check(L.pt_ctx_noise_fold(one))
        refused(g, "context 1 folded 4 groups of 12 iterations, context 0 3 of 9", 1 + 4 * G, G, 0.1, 0.25)
        g.render_features(1, 1)
        refused(g, "context 1 folded 4 groups", call="denoise_adaptive")
        assert not any(L.pt_ctx_device_counts(g.context(i)) for i in range(3))  # nobody entered the adaptive state
    finally:
        g.free()
    g = capi.Group(capi.Scene(scene_dir["cornell"], res=res), [0, 0, 0], iters_per_batch=G, convergence=2)
    try:
        warm_up(g)
        refused(g, "convergence", 1 + 2 * G, G, 0.1, 0.25)
        refused(g, "convergence", 1 + 2 * G, 10, 0.1, 0.25, call="render_threshold")
    finally:
        g.free()
