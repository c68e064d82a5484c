"""The noise estimate of the blend and the driver that stops on it, on the device (pt_history_noise, pt_history_render_until;
csrc/pt_noise.hip k_history_noise and k_noise_fold_history) against the library's host twin (the same body; pinned to the numpy
restatement by tests/test_history_noise_host.py), bit for bit.  The host twin is always fed with the renderer's own readbacks, so these
tests isolate the new code."""
import ctypes as C
import struct

import numpy as np
import pytest

import camera_scenes
import history_noise_ref as ref
import history_ref as href
import noise_ref
from history_ref import bits, f32

pytestmark = pytest.mark.gpu
RES = href.RES
VAR, MOM = 1, 2  # PT_HISTORY_VARIANCE, PT_HISTORY_MOMENTS


def same(got, want, what):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


def dbits(x):
    return struct.pack("<d", x)


def fbits(x):
    return struct.pack("<f", x)


def state_bytes(n):
    return 4 * n + 8 * ((n + 1023) // 1024 + 1)


@pytest.fixture(scope="module")
def orbit_paths(tmp_path_factory):
    return href.orbit_scene_paths(tmp_path_factory.mktemp("gpu_history_noise"), camera_scenes.cornell_text)


def first_view(r, groups=4):
    """View 0: `groups` groups of 1 with a fold after each, the features, the capture with variance."""
    for g in range(groups):
        r.render(g + 1, 1)
        r.noise_fold()
    r.render_features(1, 1)
    r.history_capture_ex(groups)


def second_view(r, capi, path, res):
    """The move to the camera of `path` and the lookup with variance: C and VC present, nothing rendered yet."""
    r.set_camera(capi.Scene(path, res=res).camera)
    r.render_features(1, 1)
    r.history_reproject_ex()


def noise_planes(r, capi):
    return capi.join_noise(r.readback_noise())


def current(r):
    return r.readback_history()[1], r.readback_history_variance()[1]


@pytest.mark.parametrize("npix", noise_ref.PIXELS)
def test_stage_equals_host(scene_dir, npix):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    Cp, VC = ref.current_planes(npix, 3 * npix)
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(32, 24)))
    try:
        for planes, M, T in ref.folded_planes(npix, (3, 1, 16), npix)[1:]:
            for cur, var, what in ((None, None, "absent"), (Cp, VC, "present")):
                w, sse = capi.stage_history_noise(planes, M, T, T, cur, var)
                want, _ = capi.history_noise_host(planes, M, T, T, cur, var)
                same(w, want, (npix, M, what))
                exact = ref.exact_sum(want)
                assert abs(sse - exact) <= 1e-9 * abs(exact), (npix, M, what, sse, exact)
                assert dbits(capi.stage_history_noise(planes, M, T, T, cur, var)[1]) == dbits(sse)  # no atomics: equal inputs, equal bits
    finally:
        r.free()


@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
@pytest.mark.parametrize("res", [(32, 24), RES], ids=["32x24", "96x54"])
def test_live_renderer_equals_host(orbit_paths, res, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    n = res[0] * res[1]
    r = capi.Renderer(capi.Scene(orbit_paths[0], res=res), arith=arith)
    try:
        first_view(r)
        second_view(r, capi, orbit_paths[1], res)
        Cp, VC = current(r)
        assert (Cp[:, 3] > 0).any() and (VC[:, :3] > 0).any() and (Cp[:, 3] == 0).any()
        T = 0
        for M, g in enumerate((2, 1, 3), start=1):
            r.render(100 + T, g)
            r.noise_fold()
            T += g
            if M < 2:
                continue
            sse = r.history_noise(T)
            want_w, want_sse = capi.history_noise_host(noise_planes(r, capi), M, T, T, Cp, VC)
            same(r.readback_history_noise(), want_w, (res, arith, M))
            exact = ref.exact_sum(want_w)
            assert abs(sse - exact) <= 1e-9 * exact and abs(want_sse - exact) <= 1e-9 * exact
            assert sse < r.noise()["sse"]  # the blend is cleaner than the view
    finally:
        r.free()


def test_without_history_it_is_the_fold_and_the_driver_is_render_until(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res, target = (32, 24), 20.0
    got = []
    for history in (True, False):
        r = capi.Renderer(capi.Scene(orbit_paths[0], res=res))
        try:
            if history:
                done, psnr, view = r.history_render_until(1, 40, target, 3)
                assert fbits(psnr) == fbits(view)
                planes = noise_planes(r, capi)
                same(r.readback_history_noise(), planes[0, :, 3], "W is the fold's .w plane")
                nz = r.noise()
                assert dbits(r.history_noise(nz["iterations"])) == dbits(nz["sse"])  # the separate launch: pt_get_noise's double
                same(r.readback_history_noise(), planes[0, :, 3], "W of the separate launch")
                assert fbits(capi.psnr_from_sse(nz["sse"], res[0] * res[1])) == fbits(psnr)
            else:
                done, psnr = r.render_until(1, 40, target, 3)
                planes = noise_planes(r, capi)
            got.append((done, fbits(psnr), r.readback(), planes))
        finally:
            r.free()
    (d0, p0, img0, pl0), (d1, p1, img1, pl1) = got
    assert d0 == d1 and 6 <= d0 < 40 and p0 == p1
    same(img0, img1, "image"), same(pl0, pl1, "planes")


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_fused_launch_equals_fold_then_estimate(orbit_paths, arith):
    """The driver's one launch per group against a second renderer stepped by hand: pt_render, pt_noise_fold, pt_history_noise."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res = RES
    n = res[0] * res[1]
    a = capi.Renderer(capi.Scene(orbit_paths[0], res=res), arith=arith)
    try:
        first_view(a)
        second_view(a, capi, orbit_paths[1], res)
        done, psnr, view = a.history_render_until(50, 7, 1000.0, 2)  # never clean: groups of 2, 2, 2, 1
        assert done == 7
        fused = (noise_planes(a, capi), a.readback_history_noise(), a.noise(), a.readback())
    finally:
        a.free()
    b = capi.Renderer(capi.Scene(orbit_paths[0], res=res), arith=arith)
    try:
        first_view(b)
        second_view(b, capi, orbit_paths[1], res)
        T = 0
        for g in (2, 2, 2, 1):
            b.render(50 + T, g)
            b.noise_fold()
            T += g
            if T > 2:
                sse = b.history_noise(T)
        nz = b.noise()
        same(fused[0], noise_planes(b, capi), "planes"), same(fused[1], b.readback_history_noise(), "W"), same(fused[3], b.readback(), "image")
        assert dbits(fused[2]["sse"]) == dbits(nz["sse"]) and fused[2]["groups"] == nz["groups"] == 4 and fused[2]["iterations"] == nz["iterations"] == 7
        assert fbits(psnr) == fbits(capi.psnr_from_sse(sse, n)) and fbits(view) == fbits(capi.psnr_from_sse(nz["sse"], n))
        assert psnr > view
    finally:
        b.free()


def test_interleaved_estimates_leave_the_fold_alone_and_memory_is_as_documented(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res = (32, 24)
    n = res[0] * res[1]
    got = []
    for estimate in (False, True):
        r = capi.Renderer(capi.Scene(orbit_paths[0], res=res))
        try:
            first_view(r)
            second_view(r, capi, orbit_paths[1], res)
            sses, bytes_ = [], []
            for g in range(4):
                r.render(20 + g, 1)
                r.noise_fold()
                if estimate and g >= 1:
                    before = r.stats().device_bytes
                    r.history_noise(g + 1)
                    bytes_.append(r.stats().device_bytes - before)
                sses.append(dbits(r.noise()["sse"]))
            if estimate:
                assert bytes_ == [state_bytes(n), 0, 0]  # the first estimate, and only that
                r.clear()
                assert r.stats().device_bytes == got[0][2] + state_bytes(n)  # kept across pt_clear
                with pytest.raises(capi.PtError, match="pt_readback_history_noise: no estimate"):
                    r.readback_history_noise()
            else:
                with pytest.raises(capi.PtError, match="pt_readback_history_noise: no estimate"):
                    r.readback_history_noise()
            got.append((noise_planes(r, capi) if not estimate else None, sses, r.stats().device_bytes))
            if not estimate:
                planes_plain = got[0][0]
        finally:
            r.free()
    # the same renderer with estimates in between: the folds' doubles are the same bits
    assert got[0][1] == got[1][1]
    # ... and so are the planes (a second pair of renderers, read before the clear)
    r = capi.Renderer(capi.Scene(orbit_paths[0], res=res))
    try:
        first_view(r)
        second_view(r, capi, orbit_paths[1], res)
        for g in range(4):
            r.render(20 + g, 1)
            r.noise_fold()
            if g >= 1:
                r.history_noise(g + 1)
        same(noise_planes(r, capi), planes_plain, "planes")
        w = r.readback_history_noise()
        r.set_camera(capi.Scene(orbit_paths[2], res=res).camera)
        with pytest.raises(capi.PtError, match="pt_readback_history_noise: no estimate"):
            r.readback_history_noise()
        assert w.shape == (n,) and (w > 0).any()
    finally:
        r.free()


@pytest.mark.parametrize("target", ref.TARGETS)
def test_the_orbit_of_the_simulation_on_the_device(orbit_paths, target):
    """The exact build reproduces the oracle's samples bit for bit, and no decision of the simulation lies within 1e-3 dB of the target,
    so the orbit of tests/test_history_noise_sim.py on the renderer takes the simulation's iterations per view under both rules."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(orbit_paths[0], res=RES), arith="exact")
    try:
        blend, alone = [], []
        for f in range(href.FRAMES):
            if f > 0:
                r.set_camera(capi.Scene(orbit_paths[f], res=RES).camera)
            alone.append(r.render_until(f * ref.CAP + 1, ref.CAP, target, ref.GROUP)[0])
            r.clear()
            r.render_features(1, 1)
            if f > 0:
                r.history_reproject_ex()
            done, psnr, view = r.history_render_until(f * ref.CAP + 1, ref.CAP, target, ref.GROUP)
            blend.append(done)
            assert abs(psnr - ref.SIM_EST_DB[target][f]) < 1e-3, (f, psnr)
            r.history_capture_ex(done)
        print(f"target {target} dB: iterations per view alone {alone}, with the blend's estimate {blend}")
        assert tuple(alone) == ref.SIM_ALONE[target] and tuple(blend) == ref.SIM_BLEND[target]
    finally:
        r.free()


def test_refusals_by_name_phrase_and_order(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    L = capi.lib()
    W = RES[0]
    d = C.c_double(0.0)

    def refused(rc, *phrases):
        assert rc != 0
        msg = L.pt_last_error().decode()
        for ph in phrases:
            assert ph in msg, (ph, msg)

    def noise(samples, flags=VAR):
        return L.pt_history_noise(C.c_float(samples), flags, C.byref(d))

    def until(first=1, count=4, group=1, target=30.0):
        return L.pt_history_render_until(first, count, group, C.c_float(target), None, None, None)

    capi.pt_free()
    refused(noise(-1.0, 7), "pt_history_noise", "pt_init")
    refused(until(0), "pt_history_render_until", "pt_init")
    refused(L.pt_readback_history_noise(None), "pt_readback_history_noise", "pt_init")
    # the flag word comes before the ragged tile; the ragged tile before everything else
    r = capi.Renderer(scene, pixel_begin=10, pixel_count=W * 3)
    try:
        before = r.stats().device_bytes
        refused(noise(-1.0, 0), "pt_history_noise", "PT_HISTORY_VARIANCE")
        refused(noise(-1.0, 3), "pt_history_noise", "PT_HISTORY_VARIANCE")
        refused(noise(-1.0, MOM), "pt_history_noise", "PT_HISTORY_MOMENTS is not built")
        refused(noise(-1.0), "pt_history_noise", "whole contiguous image rows")
        refused(until(0), "pt_history_render_until", "the first is >= 1")  # the arguments come first
        refused(until(), "pt_history_render_until", "whole contiguous image rows")
        assert r.stats().device_bytes == before
    finally:
        r.free()
    r = capi.Renderer(scene)
    try:
        before = r.stats().device_bytes
        # pt_render_until's argument check, word for word under the new name
        for args in (dict(first=0), dict(count=0), dict(group=-1), dict(target=float("inf")), dict(target=float("nan")), dict(first=2 ** 31 - 2, count=3)):
            refused(until(**args), "pt_history_render_until: iterations", "the first is >= 1, the count >= 1, the group >= 0 (0 = a batch), the target finite")
            new = L.pt_last_error().decode()
            assert L.pt_render_until(args.get("first", 1), args.get("count", 4), args.get("group", 1), C.c_float(args.get("target", 30.0)), None, None) != 0
            assert L.pt_last_error().decode().replace("pt_render_until", "pt_history_render_until") == new
        refused(noise(-1.0), "pt_history_noise", "samples")
        refused(noise(float("nan")), "pt_history_noise", "samples")
        refused(noise(4.0), "pt_history_noise", "nothing has been folded")
        assert r.stats().device_bytes == before
        r.render(1, 2)
        r.noise_fold()
        before = r.stats().device_bytes  # (the fold's planes)
        refused(noise(2.0), "pt_history_noise", "1 group(s) folded")
        r.render(3, 1)
        r.noise_fold()
        r.render(4, 1)
        refused(noise(4.0), "pt_history_noise", "fold first")
        r.noise_fold()
        refused(noise(5.0), "pt_history_noise", "samples 5", "4 iterations")
        refused(L.pt_readback_history_noise(None), "pt_readback_history_noise", "null")
        assert r.stats().device_bytes == before  # nothing allocated by any of them
        # C present with VC absent, or of the moments kind: after the folds' conditions
        r.render_features(1, 1)
        r.history_capture(4)
        r.history_reproject()
        refused(noise(5.0), "pt_history_noise", "samples 5")
        refused(noise(4.0), "pt_history_noise", "the current plane has no variance", "PT_HISTORY_VARIANCE")
        refused(until(5), "pt_history_render_until", "the current plane has no variance")
        r.clear()
        for g in range(2):
            r.render(2 * g + 1, 2)
            r.noise_fold()
        r.render_features(1, 1)
        r.history_capture_ex(4, MOM)
        r.history_reproject_ex(MOM)
        refused(noise(4.0), "pt_history_noise", "the current plane has no variance")
        refused(until(5), "pt_history_render_until", "the current plane has no variance")
        assert r.stats().device_bytes >= before and r.noise()["iterations"] == 4  # nothing was rendered by the refused drivers
        # the extra plane: the message of the other uniform-sum readers
        r.clear()
        r.render(1, 1)
        r.render_features(1, 1)
        fresh, selected = r.history_round(2, 1)
        assert selected > 0
        refused(noise(-1.0), "pt_history_noise", "extra samples", "pt_history_resolve", "pt_clear")
        refused(until(), "pt_history_render_until", "extra samples", "pt_history_resolve", "pt_clear")
        # the adaptive state comes before it
        r.clear()
        for g in range(2):
            r.render(g * 4 + 1, 4)
            r.noise_fold()
        r.adaptive_round(9, 4, 0.25)
        refused(noise(-1.0), "pt_history_noise", "adaptive state")
        refused(until(), "pt_history_render_until", "adaptive state")
    finally:
        r.free()
