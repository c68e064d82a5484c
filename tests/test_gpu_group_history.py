"""The reprojected history across a group of contexts (pt_group_history_capture_ex / _reproject_ex / _resolve / _denoise_ex / _round /
_drop, pt_group_clear, the readbacks; csrc/pt_group.cpp) and the round over a caller's list it is built on (pt_history_round_list;
csrc/pt_post.cpp): after the same calls a group holds, bit for bit, what ONE renderer of the whole frame holds.  Cornell at 97x61 (61
rows: the contexts own 31/30 and 21/20/20 of them), views 3 degrees apart at 1 spp, rounds of 3 iterations."""
import ctypes as C

import numpy as np
import pytest

from adaptive_ref import bits, f32

pytestmark = pytest.mark.gpu
G = 3
SPP = 1
RES = (97, 61)
W, H = RES
N = W * H
VAR, MOM, MOTION, FB = 1, 2, 4, 16  # PT_HISTORY_VARIANCE, _MOMENTS, _MOTION, _FEEDBACK
STEP = f32(np.pi / 60)  # 3 degrees
FRACTION = 0.25
ROW_OF = np.arange(N) // W


def visible_devices():
    import torch
    return torch.cuda.device_count()


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero((bits(a) != bits(b)).reshape(a.shape[0], -1).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:8], a[bad[:2]], b[bad[:2]])


def total_bytes(g, n):
    return sum(g.stats(i).device_bytes for i in range(n)) + g.device_bytes()


def context_samples(g, n):
    return [g.stats(i).samples for i in range(n)]


def same_state(g, r, n, what, captured):
    """The gathered image, the four history planes, E and the sample counts of a group against one renderer's."""
    same_bits(g.gather(), r.readback(), (what, "image"))
    same_bits(g.readback_history_extra(), r.readback_history_extra(), (what, "E"))
    if captured:
        (gk, gc), (rk, rc) = g.readback_history(), r.readback_history()
        same_bits(gk.reshape(-1, 4), rk.reshape(-1, 4), (what, "K"))
        same_bits(gc, rc, (what, "C"))
    (gvk, gvc), (rvk, rvc) = g.readback_history_variance(), r.readback_history_variance()
    same_bits(gvk, rvk, (what, "VK"))
    same_bits(gvc, rvc, (what, "VC"))
    assert sum(context_samples(g, n)) == r.stats().samples, what


def both(r, g):
    return (r, g)


# ---- (1) a round over a caller's list ------------------------------------------------------------------------------------------------------
def list_round_inputs(capi, scene, kw):
    """One whole-frame renderer after pt_history_round, and the list its selection made (from pt_history_select_host on its readbacks)."""
    emitter = capi.emitter_geoms(scene)
    cap = capi.history_list_capacity(FRACTION, N)
    r = capi.Renderer(scene, **kw)
    try:
        r.render(1, SPP)
        r.render_features(1, 1)
        lst, fresh, m = capi.history_select_host(r.readback_feature_planes(), W, H, None, emitter, max_fraction=FRACTION)
        assert r.history_round(2, G, max_fraction=FRACTION) == (fresh, m) and m == cap < fresh
        return np.asarray(lst[:m], np.int32), cap, dict(S=r.readback(), E=r.readback_history_extra(), samples=r.stats().samples)
    finally:
        r.free()


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_round_list_equals_history_round(scene_dir, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    L = capi.lib()
    scene = capi.Scene(scene_dir["cornell"], res=RES)
    kw = dict(arith=arith, iters_per_batch=G)
    lst, cap, want = list_round_inputs(capi, scene, kw)
    assert np.array_equal(np.flatnonzero(want["E"]), lst) and (want["E"][lst] == G).all()
    # (a) the same list on a twin renderer
    r = capi.Renderer(scene, **kw)
    try:
        r.render(1, SPP)
        r.history_round_list(2, G, lst, cap)
        same_bits(r.readback(), want["S"], "S"), same_bits(r.readback_history_extra(), want["E"], "E")
        assert r.stats().samples == want["samples"]
        r.history_round_list(2 + G, G, lst[:0], cap)  # an empty list renders nothing and keeps E
        same_bits(r.readback(), want["S"], "S, empty list"), same_bits(r.readback_history_extra(), want["E"], "E, empty list")
        assert r.stats().samples == want["samples"]
    finally:
        r.free()
    # (b) the striped tiles of a two-context group, each context over its part of the list
    g = capi.Group(scene, [0, 0], **kw)
    try:
        g.render(1, SPP)
        parts, counts = capi.group_partition_host(lst, W, H, 2)
        assert counts.sum() == lst.size and counts.min() > 0
        for i in range(2):
            pixels = ((H - i + 1) // 2) * W
            part = np.ascontiguousarray(parts[i], np.int32)
            capi._check(L.pt_ctx_history_round_list(g.context(i), 2, G, capi._i(part), part.size, min(cap, pixels)))
            S, E = np.empty((pixels, 3), f32), np.empty(pixels, f32)
            capi._check(L.pt_ctx_readback(g.context(i), capi._f(S)))
            capi._check(L.pt_ctx_readback_history_extra(g.context(i), capi._f(E)))
            rows = ROW_OF % 2 == i
            same_bits(S, want["S"][rows], ("rows of context", i, "S")), same_bits(E, want["E"][rows], ("rows of context", i, "E"))
        same_bits(g.gather(), want["S"], "gathered S"), same_bits(g.readback_history_extra(), want["E"], "gathered E")
        assert sum(context_samples(g, 2)) == want["samples"]
    finally:
        g.free()


def test_round_list_refuses(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    w, h = 33, 9
    scene = capi.Scene(scene_dir["cornell"], res=(w, h))

    def refused(r, match, first, iters, lst, capacity):
        before = r.stats().device_bytes
        with pytest.raises(capi.PtError, match="pt_history_round_list: .*" + match):
            r.history_round_list(first, iters, np.array(lst, np.int32), capacity)
        assert r.stats().device_bytes == before, match

    r = capi.Renderer(scene, iters_per_batch=G)
    try:
        refused(r, "iterations 0", 0, G, [0], 0)  # the iterations come before the capacity
        refused(r, "at least one", 1, 0, [0], 0)
        refused(r, "iterations", 2 ** 31 - 2, 3, [0], 0)
        refused(r, "a worker for 0", 1, G, [], 0)
        refused(r, f"a worker for {w * h + 1}", 1, G, [0], w * h + 1)
        refused(r, "a list of 3 on a worker for 2", 1, G, [0, 1, 2], 2)
        refused(r, r"list\[2\] = 1 ", 1, G, [0, 1, 1], 4)
        refused(r, r"list\[1\] = 0 ", 1, G, [5, 0], 4)
        refused(r, rf"list\[0\] = {w * h} ", 1, G, [w * h], 4)
        before = r.stats().device_bytes
        assert capi.lib().pt_history_round_list(1, G, None, 1, 1) != 0 and "null list" in capi.lib().pt_last_error().decode()
        assert r.stats().device_bytes == before and not r.readback_history_extra().any()
        for k in range(2):  # the adaptive state comes before the capacity
            r.render(1 + k * G, G)
            r.noise_fold()
        r.adaptive_round(1 + 2 * G, G, 0.25)
        refused(r, "adaptive state", 1 + 3 * G, G, [0], 0)
    finally:
        r.free()
    r = capi.Renderer(scene, iters_per_batch=G, convergence=2)
    try:
        refused(r, "iterations 0", 0, G, [0], 1)  # ... and before the convergence metric
        refused(r, "convergence", 1, G, [0], 0)
    finally:
        r.free()


# ---- (2), (3) the orbit ----------------------------------------------------------------------------------------------------------------------
def orbit(scene_dir, devices, arith, flags, rounds):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(scene_dir["cornell"], res=RES)
    kw = dict(arith=arith, iters_per_batch=G)
    n = len(devices)
    r = capi.Renderer(scene, **kw)
    g = capi.Group(scene, devices, **kw)
    try:
        selected = []
        for f in range(3):
            what = (devices, arith, flags, f)
            if f > 0:
                cam = scene.orbit(STEP, 0.0, 0.0)
                for x in both(r, g):
                    x.set_camera(cam)
            first = 4 * f + 1
            for x in both(r, g):
                x.render(first, SPP)
                x.render_features(1, 1)
                if f > 0:
                    x.history_reproject_ex(flags)
            same_state(g, r, n, (what, "lookup"), f > 0)
            if f > 0:
                assert g.readback_history()[1][:, 3].any(), what  # something was carried
            if rounds:  # the first view has no history: the cap cuts its list; later views select the pixels that carry less than one sample
                opts = dict(max_fraction=FRACTION, min_history=0.0 if f == 0 else 0.75)
                want = r.history_round(first + 1, G, **opts)
                got = g.history_round(first + 1, G, **opts)
                assert got == want and 0 < got[1] <= got[0], (what, got, want)
                selected.append(got[1])
                same_state(g, r, n, (what, "round"), f > 0)
                assert g.readback_history_extra().any(), what
            same_bits(g.history_resolve(SPP), r.history_resolve(SPP), (what, "blend"))
            if flags:
                same_bits(g.history_denoise_ex(SPP), r.history_denoise_ex(SPP), (what, "filtered"))
                same_bits(g.history_denoise_ex(SPP, levels=3, keep_albedo=True), r.history_denoise_ex(SPP, levels=3, keep_albedo=True), (what, "filtered, 3 levels"))
            for x in both(r, g):
                x.history_capture_ex(SPP, flags)
            same_state(g, r, n, (what, "capture"), True)
        if rounds:
            assert selected[0] == int(np.ceil(FRACTION * N)), selected
    finally:
        g.free()
        r.free()


@pytest.mark.parametrize("contexts", [2, 3])
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_orbit_with_moments_equals_single_context(scene_dir, contexts, arith):
    orbit(scene_dir, [0] * contexts, arith, MOM, True)


@pytest.mark.parametrize("contexts", [2, 3])
def test_orbit_plain_equals_single_context(scene_dir, contexts):
    orbit(scene_dir, [0] * contexts, "fma", 0, False)


def test_orbit_on_every_visible_device(scene_dir):
    """The RCCL branch of the exchanges: the image, the planes and E to the root, the parts back."""
    ndev = visible_devices()
    if ndev < 2:
        pytest.skip("one visible device: the RCCL exchanges need two")
    orbit(scene_dir, list(range(ndev)), "exact", MOM, True)


# ---- (4) a part that is empty ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contexts", [2, 3])
def test_round_with_empty_parts(scene_dir, contexts):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    L = capi.lib()
    scene = capi.Scene(scene_dir["cornell"], res=RES)
    kw = dict(arith="exact", iters_per_batch=G)
    r = capi.Renderer(scene, **kw)
    g = capi.Group(scene, [0] * contexts, **kw)
    try:
        for x in both(r, g):
            x.render(1, SPP)
            x.render_features(1, 1)
        before = context_samples(g, contexts)
        want = r.history_round(2, G, max_fraction=1.0 / N)  # cap 1
        got = g.history_round(2, G, max_fraction=1.0 / N)
        assert got == want and got[1] == 1 < got[0], (got, want)
        grew = [a - b for a, b in zip(context_samples(g, contexts), before)]
        assert sorted(grew) == [0] * (contexts - 1) + [G], grew  # one context renders the pixel, the others nothing ...
        for i in range(contexts):  # ... and all of them hold E: what reads a uniform SUM refuses on every context
            assert L.pt_ctx_noise_fold(g.context(i)) != 0 and "pt_history_resolve" in L.pt_last_error().decode(), i
        same_state(g, r, contexts, "round of one pixel", False)
        assert np.count_nonzero(g.readback_history_extra()) == 1
        same_bits(g.history_resolve(SPP), r.history_resolve(SPP), "blend")
        for x in both(r, g):
            x.history_capture_ex(SPP, MOM)
        same_state(g, r, contexts, "capture", True)
    finally:
        g.free()
        r.free()


# ---- (5) objects that move ----------------------------------------------------------------------------------------------------------------------
def test_motion_equals_single_context(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(scene_dir["cornell"], res=RES)
    sphere = [i for i, geom in enumerate(scene.geoms()) if geom.type == 0][0]  # PT_GEOM_SPHERE
    kw = dict(arith="exact", iters_per_batch=G)
    r = capi.Renderer(scene, **kw)
    g = capi.Group(scene, [0, 0, 0], **kw)
    try:
        for x in both(r, g):
            x.render(1, SPP)
            x.render_features(1, 1)
            x.history_capture_ex(SPP, MOM)
        trs = scene.geom_trs(sphere)
        trs[0] += f32(0.5)
        scene.set_geom_trs(sphere, trs)
        planes = {}
        for x in both(r, g):
            x.set_geoms(scene)
            x.render(2, SPP)
            x.render_features(1, 1)
        # (cornell's sphere is a mirror, which carries nothing unless keep_view_dependent is set: with it the flag shows in C)
        for keep in (False, True):
            for flags in (MOM | MOTION, MOM, MOTION, 0):
                for x in both(r, g):
                    x.history_reproject_ex(flags, keep_view_dependent=keep)
                same_state(g, r, 3, ("lookup", flags, keep), True)
                planes[flags] = g.readback_history()[1]
        assert (bits(planes[MOM | MOTION]) != bits(planes[MOM])).any()  # the flag follows the sphere; without it the world is static
        assert (bits(planes[MOTION]) != bits(planes[0])).any()
        for x in both(r, g):  # the capture retakes the geoms: nothing has moved since, and the lookup with the flag is the static one
            x.history_reproject_ex(MOM | MOTION)
            x.history_capture_ex(SPP, MOM)
            x.clear()
            x.render(3, SPP)
            x.render_features(1, 1)
            x.history_reproject_ex(MOM | MOTION)
        same_state(g, r, 3, "lookup after the capture", True)
    finally:
        g.free()
        r.free()


# ---- (6) lifetimes --------------------------------------------------------------------------------------------------------------------------------
def test_lifetimes(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(scene_dir["cornell"], res=RES)
    kw = dict(arith="exact", iters_per_batch=G)
    r = capi.Renderer(scene, **kw)
    g = capi.Group(scene, [0, 0], **kw)

    def view(first):
        for x in both(r, g):
            x.render(first, SPP)
            x.render_features(1, 1)

    def absent(what):
        """C and VC are absent, K stays: the resolve is S / samples."""
        view(50)
        same_state(g, r, 2, what, True)
        kept, cur = g.readback_history()
        assert not cur.any() and not g.readback_history_variance()[1].any() and kept.any(), what
        same_bits(g.history_resolve(SPP), capi.history_blend_host(g.gather(), SPP, None), (what, "S / samples"))
        for x in both(r, g):
            x.history_reproject_ex(MOM)
        same_state(g, r, 2, (what, "the lookup after it"), True)
        assert g.readback_history()[1].any(), what

    try:
        view(1)
        for x in both(r, g):
            x.history_capture_ex(SPP, MOM)
            x.history_reproject_ex(MOM)
        assert g.readback_history()[1].any()
        for x in both(r, g):
            x.clear()
        absent("pt_group_clear")
        cam = scene.orbit(STEP, 0.0, 0.0)
        for x in both(r, g):
            x.set_camera(cam)
        absent("pt_group_set_camera")
        cam = scene.orbit(STEP, 0.0, 0.0)
        for x in both(r, g):
            x.set_camera(cam, device_tables=True)
        absent("pt_group_set_camera_ex")
        for x in both(r, g):
            x.set_geoms(scene)
        absent("pt_group_set_geoms")
        # a plain capture after a moments capture: kept without moments
        for x in both(r, g):
            x.history_capture_ex(SPP, 0)
        with pytest.raises(capi.PtError, match="pt_group_history_reproject_ex: nothing has been captured with moments"):
            g.history_reproject_ex(MOM)
        for x in both(r, g):
            x.history_reproject_ex(0)
        same_state(g, r, 2, "plain lookup", True)
        # the drop forgets everything and keeps the memory
        before = total_bytes(g, 2)
        for x in both(r, g):
            x.history_drop()
        assert total_bytes(g, 2) == before
        same_state(g, r, 2, "drop", True)
        assert not g.readback_history()[0].any()
        with pytest.raises(capi.PtError, match="pt_group_history_reproject_ex: nothing has been captured"):
            g.history_reproject_ex(0)
    finally:
        g.free()
        r.free()


# ---- (7) refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_order_allocate_nothing(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    L = capi.lib()
    n = 3
    scene = capi.Scene(scene_dir["cornell"], res=(33, 9))

    def refused(g, call, match, *args, **kw):
        before = total_bytes(g, n)
        with pytest.raises(capi.PtError, match=f"pt_group_{call}: .*{match}"):
            getattr(g, call)(*args, **kw)
        assert total_bytes(g, n) == before, (call, match)

    g = capi.Group(scene, [0] * n, iters_per_batch=G)
    try:
        g.render(1, SPP)
        # an undefined flag bit, then the feature pass, then the samples and the options, then what a group does not have
        refused(g, "history_capture_ex", "undefined flag bit", -1.0, 8)
        refused(g, "history_capture_ex", "undefined flag bit", -1.0, MOTION)
        refused(g, "history_capture_ex", "exclude each other", -1.0, VAR | MOM)
        refused(g, "history_capture_ex", "PT_HISTORY_FEEDBACK needs PT_HISTORY_MOMENTS", -1.0, FB)
        refused(g, "history_reproject_ex", "undefined flag bit", 8, cap=-1.0)
        refused(g, "history_denoise_ex", "undefined flag bit", -1.0, VAR)
        refused(g, "history_capture_ex", "no feature pass", -1.0, VAR)
        refused(g, "history_reproject_ex", "no feature pass", VAR, cap=-1.0)
        refused(g, "history_denoise_ex", "no feature pass", -1.0, 0)
        refused(g, "history_round", "iterations 0", 0, 1, -1.0)
        refused(g, "history_round", "at least one", 1, 0, -1.0)
        refused(g, "history_round", "no feature pass", 1, 1, -1.0)
        refused(g, "history_resolve", "samples must be finite and positive", 0.0)  # (the resolve needs no feature pass)
        g.render_features(1, 1)
        for samples in (0.0, -1.0, float("nan"), float("inf")):
            refused(g, "history_capture_ex", "samples must be finite and positive", samples, VAR)
            refused(g, "history_denoise_ex", "samples must be finite and positive", samples, 0, levels=9)
            refused(g, "history_resolve", "samples must be finite and positive", samples)
        refused(g, "history_reproject_ex", "cap must be positive", VAR, cap=-1.0)
        refused(g, "history_reproject_ex", "not finite", MOM | FB, plane_tol=float("nan"))
        refused(g, "history_denoise_ex", "levels", SPP, 0, levels=9)
        refused(g, "history_round", "min_history", 1, 1, -1.0)
        refused(g, "history_round", "max_fraction", 1, 1, 0.0, 1.5)
        refused(g, "history_capture_ex", "PT_HISTORY_VARIANCE is not built for a group", SPP, VAR)
        refused(g, "history_capture_ex", "PT_HISTORY_FEEDBACK is not built for a group", SPP, MOM | FB)
        refused(g, "history_reproject_ex", "PT_HISTORY_VARIANCE is not built for a group", VAR)
        refused(g, "history_reproject_ex", "PT_HISTORY_VARIANCE is not built for a group", VAR | MOTION)
        refused(g, "history_reproject_ex", "PT_HISTORY_FEEDBACK is not built for a group", MOM | FB)
        refused(g, "history_denoise_ex", "not built for a group", SPP, 0)
        # nothing captured, nothing captured with moments, a C of another kind
        refused(g, "history_reproject_ex", "nothing has been captured", 0)
        refused(g, "history_reproject_ex", "nothing has been captured", MOM | MOTION)
        refused(g, "readback_history", "nothing has been captured")
        g.history_capture_ex(SPP, 0)
        refused(g, "history_reproject_ex", "nothing has been captured with moments", MOM)
        g.history_reproject_ex(0)
        refused(g, "history_capture_ex", "the current plane has no moments", SPP, MOM)
        refused(g, "history_denoise_ex", "the current plane has no moments", SPP, MOM)
        g.history_capture_ex(SPP, 0), g.history_resolve(SPP)  # these read C alone
        # a caller who runs a round on ONE context breaks the group: the contexts disagree on E
        one = np.array([0], np.int32)
        capi._check(L.pt_ctx_history_round_list(g.context(1), 2, G, capi._i(one), 1, 1))
        g.history_reproject_ex(0)  # (the lookup reads no E)
        for call, args in (("history_capture_ex", (SPP, 0)), ("history_resolve", (SPP,)), ("history_round", (2 + G, G)), ("readback_history_extra", ())):
            refused(g, call, "context 1 holds the extra plane of the history round, context 0 does not", *args)
        g.clear()
        assert not g.readback_history_extra().any()
    finally:
        g.free()
    # the adaptive state comes before the feature pass; the convergence metric before both
    g = capi.Group(scene, [0] * n, iters_per_batch=G)
    try:
        for k in range(2):
            g.render(1 + k * G, G)
            g.noise_fold()
        above, m = g.adaptive_round_threshold(1 + 2 * G, G, 0.0, 0.25)
        assert m > 0
        refused(g, "history_capture_ex", "adaptive state", -1.0, VAR)
        refused(g, "history_capture_ex", "undefined flag bit", -1.0, 8)  # (the flag word comes before the state)
        refused(g, "history_reproject_ex", "adaptive state", VAR, cap=-1.0)
        refused(g, "history_resolve", "adaptive state", -1.0)
        refused(g, "history_denoise_ex", "adaptive state", -1.0, 0)
        refused(g, "history_round", "adaptive state", 1, 1, -1.0)
        refused(g, "history_round", "iterations 0", 0, 1, -1.0)
    finally:
        g.free()
    g = capi.Group(scene, [0] * n, iters_per_batch=G, convergence=2)
    try:
        refused(g, "history_round", "iterations 0", 0, 1, -1.0)
        refused(g, "history_round", "convergence", 1, 1, -1.0)
    finally:
        g.free()


def test_what_reads_a_uniform_sum_refuses_while_extras_are_present(scene_dir):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = 2
    g = capi.Group(capi.Scene(scene_dir["cornell"], res=(33, 9)), [0] * n, iters_per_batch=G)
    try:
        for k in range(2):
            g.render(1 + k, 1)
            g.noise_fold()
        g.render_features(1, 1)
        g.denoise_guided(), g.resolve(), g.gather_u8(2), g.preview(2)  # all fine before the round
        fresh, m = g.history_round(100, G)
        assert m > 0
        before = total_bytes(g, n)
        calls = {
            "denoise": lambda: g.denoise(2),
            "denoise_guided": g.denoise_guided,
            "denoise_adaptive": g.denoise_adaptive,
            "noise_fold": g.noise_fold,
            "render_until": lambda: g.render_until(200, 4, 30.0, 2),
            "adaptive_round_threshold": lambda: g.adaptive_round_threshold(200, 2, 0.01, 0.25),
            "render_threshold": lambda: g.render_threshold(200, 4, 0.01, 0.25, 2),
            "resolve": g.resolve,
            "gather_u8": lambda: g.gather_u8(2),
            "preview": lambda: g.preview(2),
        }
        samples = context_samples(g, n)
        for name, call in calls.items():
            with pytest.raises(capi.PtError) as e:
                call()
            msg = str(e.value)
            assert "left extra samples" in msg and "pt_history_resolve" in msg and "pt_clear" in msg, (name, msg)
        assert total_bytes(g, n) == before and context_samples(g, n) == samples  # nothing allocated, nothing rendered
        # these keep working
        g.gather(), g.history_resolve(2), g.history_capture_ex(2, MOM), g.history_denoise_ex(2)
        g.clear()
        g.render(1, 1)
        g.noise_fold()  # back in the uniform state
        g.resolve()
    finally:
        g.free()
