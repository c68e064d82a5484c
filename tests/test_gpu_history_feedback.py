"""The feedback on the device (pt_history_reproject_ex / _capture_ex with PT_HISTORY_FEEDBACK, pt_history_denoise_feedback;
csrc/pt_history.hip k_history_reproject_feedback, csrc/pt_denoise.hip k_denoise_prepare_feedback and k_history_feedback_tap) against the
library's host functions (the same bodies; pinned to the numpy restatement by tests/test_history_feedback_host.py), bit for bit.  The
host functions are always fed with the renderer's own readbacks, so these tests isolate the new code."""
import ctypes as C

import numpy as np
import pytest

import camera_scenes
import denoise_ref
import history_feedback_ref as ref
import history_moments_ref as mref
import history_ref as href
import history_round_ref as rref
from history_ref import bits, f32

pytestmark = pytest.mark.gpu
RES = href.RES
W, H = RES
N = W * H
VAR, MOM, MOTION, FB = 1, 2, 4, 16  # PT_HISTORY_VARIANCE, _MOMENTS, _MOTION, _FEEDBACK
SPP = 1


def same(got, want, what):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


@pytest.fixture(scope="module")
def orbit_paths(tmp_path_factory):
    return href.orbit_scene_paths(tmp_path_factory.mktemp("gpu_history_feedback"), camera_scenes.cornell_text)


@pytest.mark.parametrize("arith", ["exact", "fma", "fast"])
def test_stage_equals_host(scene_dir, arith):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_dir["cornell"], res=(32, 24)), arith=arith)
    try:
        for shape in ref.SHAPES:
            w, rows, row0, _ = shape
            n = w * rows
            cam, kept, feat, reject, table, kind, vk, fk = ref.lookup_arrays(*shape)
            for mo in (dict(), dict(table=table, kind=kind)):
                for opts in (dict(), dict(cap=8.0, min_normal_dot=0.5, plane_tol=0.25), dict(keep_view_dependent=True)):
                    got = capi.stage_history_reproject_feedback(cam.to_capi(), kept, feat, reject, vk, fk, w, rows, row0, **mo, **opts)
                    want = capi.history_reproject_feedback_host(cam.to_capi(), kept, feat, reject, vk, fk, w, rows, row0, **mo, **opts)
                    for a, b, what in zip(got, want, ("C", "VC", "FC")):
                        same(a, b, (w, rows, bool(mo), opts, what))
            if n > 100:
                assert (want[2][:, 3] > 0).any()
            S, planes = denoise_ref.random_frame(w, rows, SPP)
            Cp, VC, FC = ref.current_planes(n, 3 * n)
            for levels in (1, 2, 3):
                for level in sorted({1, levels}):
                    for variance in (0, 1):
                        for E in (None, ref.extra_plane(n, n)):
                            opts = dict(levels=levels, level=level, variance=variance, keep_albedo=(levels == 2))
                            got = capi.stage_history_denoise_feedback(S, planes, w, rows, SPP, E, Cp, VC, FC, **opts)
                            want = capi.history_denoise_feedback_host(S, planes, w, rows, SPP, E, Cp, VC, FC, **opts)
                            same(got[0], want[0], (w, rows, opts, E is not None, "filtered")), same(got[1], want[1], (w, rows, opts, E is not None, "tap"))
            got = capi.stage_history_denoise_feedback(S, planes, w, rows, SPP)
            same(got[0], capi.history_denoise_moments_host(S, planes, w, rows, SPP), (w, rows, "history absent, default options: the moments filter"))
            same(got[1], capi.history_denoise_feedback_host(S, planes, w, rows, SPP)[1], (w, rows, "... and its tap"))
    finally:
        r.free()


def sequence(capi, r, paths, views, feedback, extra=0, sim_numbers=False, **fb):
    """The command line's order through `views` views at 1 spp — render, features, lookup, round, resolve, filter, capture, move — with
    or without PT_HISTORY_FEEDBACK: per view everything the renderer read back.  sim_numbers: the iteration numbers of
    tests/test_history_feedback_sim.py (view f renders iteration f + 1, its round 1000 + f G + 1 ..) in place of the command line's."""
    flags = MOM | (FB if feedback else 0)
    out = []
    for f in range(views):
        cam = capi.Scene(paths[f], res=RES).camera
        if f > 0:
            r.set_camera(cam)
        first = f + 1 if sim_numbers else f * (SPP + extra) + 1
        r.render(first, SPP)
        r.render_features(1, 1)
        v = dict(cam=cam, feat=r.readback_feature_planes())
        if f > 0:
            r.history_reproject_ex(flags)
            v["C"] = r.readback_history()[1]
        else:  # nothing captured yet: pt_readback_history refuses
            v["C"] = np.zeros((N, 4), f32)
        v["VC"] = r.readback_history_variance()[1]
        v["FC"] = r.readback_history_feedback()[1]
        if extra:
            v["round"] = r.history_round(1000 + f * extra + 1 if sim_numbers else first + SPP, extra)
        v["E"], v["S"] = r.readback_history_extra(), r.readback()
        v["blend"] = r.history_resolve(SPP)
        v["filtered"] = r.history_denoise_feedback(SPP, **fb) if feedback else r.history_denoise_ex(SPP)
        v["P"] = r.readback_history_feedback()[2]
        r.history_capture_ex(SPP, flags)
        v["K"], v["VK"] = r.readback_history()[0], r.readback_history_variance()[0]
        v["FK"], _, v["P_after"] = r.readback_history_feedback()
        v["bytes"] = r.stats().device_bytes
        out.append(v)
    return out


def check_against_host(capi, scene, seq, extra, level, variance):
    reject = capi.reject_geoms(scene)
    prev = None
    for f, v in enumerate(seq):
        S, feat, E = v["S"], v["feat"], v["E"] if extra else None
        Cp = VC = FC = None
        if prev is not None:
            Cp, VC, FC = capi.history_reproject_feedback_host(prev["cam"], prev["K"], feat, reject, prev["VK"], prev["FK"], W, H)
            same(v["C"], Cp, (f, "C")), same(v["VC"], VC, (f, "VC")), same(v["FC"], FC, (f, "FC"))
            assert (FC[:, 3] > 0).any() and (FC[:, :3] > 0).any()
        else:
            assert not v["C"].any() and not v["VC"].any() and not v["FC"].any()
        filtered, P = capi.history_denoise_feedback_host(S, feat, W, H, SPP, E, Cp, VC, FC, level=level, variance=variance)
        same(v["filtered"], filtered, (f, "pt_history_denoise_feedback")), same(v["P"], P, (f, "P"))
        K = capi.history_capture_host(S, feat, SPP, Cp) if E is None else capi.history_capture_counted_host(S, feat, SPP, E, Cp)
        VK = capi.history_capture_moments_host(S, SPP, Cp, VC) if E is None else capi.history_capture_moments_counted_host(S, SPP, E, Cp, VC)
        same(v["K"], K, (f, "K")), same(v["VK"], VK, (f, "VK"))
        same(v["FK"], P, (f, "FK := P")),
        assert not v["P_after"].any()  # promoted: the pending plane is absent again
        prev = v
    assert (seq[-1]["FK"][:, 3] > 0).any()


@pytest.mark.parametrize("extra,level,variance", [(0, 0, None), (3, 2, 0)], ids=["defaults", "rounds-L2-rule0"])
def test_renderer_sequence_equals_host_and_leaves_the_raw_chain_alone(orbit_paths, extra, level, variance):
    """Four views of the orbit.  Every plane after every step equals the host functions' fed with the read-back inputs; and a second
    renderer that makes the same calls without the flag reads back the same K, VK, C, VC, E and blend at every view, bit for bit —
    with rounds composed in, whose lists are therefore the same — and never allocates the feedback's 48 bytes per pixel."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    seqs = []
    for feedback in (True, False):
        r = capi.Renderer(scene, arith="exact")
        try:
            seqs.append(sequence(capi, r, orbit_paths, 4, feedback, extra, level=level, variance=variance) if feedback else sequence(capi, r, orbit_paths, 4, False, extra))
        finally:
            r.free()
    with_fb, without = seqs
    check_against_host(capi, scene, with_fb, extra, level, variance)
    for f, (a, b) in enumerate(zip(with_fb, without)):
        for name in ("K", "VK", "C", "VC", "E", "S", "blend"):
            same(a[name], b[name], (f, name, "the raw chain"))
        assert a.get("round") == b.get("round")
        assert not b["FC"].any() and not b["P"].any() and not b["FK"].any()
        assert a["bytes"] - b["bytes"] == 48 * N, (f, a["bytes"], b["bytes"])
        assert (bits(a["filtered"]) != bits(b["filtered"])).any() == (f > 0)  # the first view has no history to differ in
    if extra:
        assert all(v["round"][1] > 0 for v in with_fb) and with_fb[1]["E"].any()


def test_the_orbit_of_the_simulation_on_the_device(orbit_paths):
    """The exact build reproduces the oracle's samples bit for bit, so the orbit of tests/test_history_feedback_sim.py run on the
    renderer with the library's defaults gives the simulation's figure; the 1024-spp frame at the last camera comes from the renderer."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(orbit_paths[0], res=RES), arith="exact")
    try:
        plain = sequence(capi, r, orbit_paths, href.FRAMES, True)
    finally:
        r.free()
    r = capi.Renderer(capi.Scene(orbit_paths[0], res=RES), arith="exact")
    try:
        rounds = sequence(capi, r, orbit_paths, href.FRAMES, True, rref.SIM_GROUP, sim_numbers=True)
    finally:
        r.free()
    r = capi.Renderer(capi.Scene(orbit_paths[-1], res=RES), arith="exact")
    try:
        r.render(href.TRUTH_FIRST, href.TRUTH_SPP)
        truth = r.readback().astype(np.float64) / href.TRUTH_SPP
    finally:
        r.free()
    L, V = ref.DEFAULTS
    got = href.mse(plain[-1]["filtered"], truth)
    print(f"orbit at 1 spp with feedback (level {L}, rule {V}) on the device, last view: MSE of the filtered image {got:.9g} "
          f"(without feedback {mref.SIM_FILTERED:.9g})")
    assert abs(got / ref.SIM_ORBIT[L - 1][V] - 1) < 1e-6, (got, ref.SIM_ORBIT[L - 1][V])
    got = href.mse(rounds[-1]["filtered"], truth)
    print(f"... with rounds of {rref.SIM_GROUP}: {got:.9g} (without feedback {rref.SIM_ROUND_FILTERED:.9g}); lists {[v['round'][1] for v in rounds]}")
    assert abs(got / ref.SIM_ROUNDS[L - 1][V] - 1) < 1e-6, (got, ref.SIM_ROUNDS[L - 1][V])
    assert [v["round"][1] for v in rounds] == rref.SIM_ROUND_M  # the raw chain's lists: those of the orbit without feedback


def one_view(r, first=1):
    r.render(first, 1)
    r.render_features(1, 1)


def test_lifetime_of_the_three_planes(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    r = capi.Renderer(scene)
    try:
        one_view(r)
        r.history_denoise_ex(SPP)  # (the shared workspace, so that it is not counted below)
        r.history_capture_ex(SPP, MOM)
        r.history_reproject_ex(MOM)
        before = r.stats().device_bytes
        assert not any(p.any() for p in r.readback_history_feedback())
        assert r.stats().device_bytes == before  # a readback allocates nothing
        with pytest.raises(capi.PtError, match="pt_history_denoise_feedback: the current plane has no filtered colour"):
            r.history_denoise_feedback(SPP)
        r.clear(), one_view(r)
        assert r.stats().device_bytes == before
        out = r.history_denoise_feedback(SPP, levels=2, level=2)
        assert r.stats().device_bytes - before == 48 * N  # the first call that carries the feedback, and only that
        fk, fc, p = r.readback_history_feedback()
        assert not fk.any() and not fc.any()
        same(p[:, :3], out, "L == levels: the tap's xyz are the output")
        # P becomes absent on pt_render, pt_render_features and pt_history_round
        r.render(2, 1)
        assert not r.readback_history_feedback()[2].any()
        with pytest.raises(capi.PtError, match="pt_history_capture_ex: the pending plane is absent: filter first .pt_history_denoise_feedback"):
            r.history_capture_ex(2, MOM | FB)
        r.history_denoise_feedback(2)
        assert r.readback_history_feedback()[2].any()
        r.render_features(1, 1)
        assert not r.readback_history_feedback()[2].any()
        r.history_denoise_feedback(2)
        r.history_round(3, 2)
        assert not r.readback_history_feedback()[2].any()
        r.history_denoise_feedback(2)
        p = r.readback_history_feedback()[2]
        r.history_capture_ex(2, MOM | FB)
        fk, fc, pend = r.readback_history_feedback()
        same(fk, p, "FK := P"), same(r.readback_history_feedback()[0], fk, "")
        assert not fc.any() and not pend.any()
        r.history_reproject_ex(MOM | FB)
        assert r.readback_history_feedback()[1].any()
        # FC absent and FK kept after pt_clear, pt_set_camera and pt_set_geoms
        r.clear()
        kept, cur, pend = r.readback_history_feedback()
        same(kept, fk, "FK survives pt_clear"), same(cur, np.zeros_like(cur), "FC"), same(pend, np.zeros_like(cur), "P")
        for move in (lambda: r.set_camera(capi.Scene(orbit_paths[1], res=RES).camera), lambda: r.set_geoms(scene)):
            one_view(r)
            r.history_reproject_ex(MOM | FB)
            r.history_denoise_feedback(SPP)
            assert all(pl.any() for pl in r.readback_history_feedback())
            move()
            kept, cur, pend = r.readback_history_feedback()
            same(kept, fk, "FK survives the move"), same(cur, np.zeros_like(cur), "FC"), same(pend, np.zeros_like(cur), "P")
        # a lookup without the flag leaves FC absent; a capture without it leaves K kept without feedback
        one_view(r)
        r.history_reproject_ex(MOM)
        assert not r.readback_history_feedback()[1].any()
        r.history_capture_ex(SPP, MOM)
        assert not r.readback_history_feedback()[0].any()
        with pytest.raises(capi.PtError, match="pt_history_reproject_ex: nothing has been captured with feedback"):
            r.history_reproject_ex(MOM | FB)
        # pt_history_drop forgets all three
        r.history_reproject_ex(MOM)
        with pytest.raises(capi.PtError, match="no filtered colour"):
            r.history_denoise_feedback(SPP)
        r.clear(), one_view(r)
        r.history_denoise_feedback(SPP)
        r.history_capture_ex(SPP, MOM | FB)
        r.history_reproject_ex(MOM | FB)
        r.history_denoise_feedback(SPP)
        assert all(pl.any() for pl in r.readback_history_feedback())
        r.history_drop()
        assert not any(pl.any() for pl in r.readback_history_feedback())
    finally:
        r.free()


def test_refusals_by_name_phrase_and_order(orbit_paths):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(orbit_paths[0], res=RES)
    L = capi.lib()
    buf = np.empty((N, 3), f32)
    p = capi._f(buf)
    one = C.c_float(1.0)

    def refused(rc, *phrases):
        assert rc != 0
        msg = L.pt_last_error().decode()
        for ph in phrases:
            assert ph in msg, (ph, msg)

    def fbo(level=0, variance=0):
        return C.byref(capi.PtHistoryFeedbackOptions(level, variance))

    who = "pt_history_denoise_feedback"
    capi.pt_free()
    refused(L.pt_history_denoise_feedback(one, None, None, None), who, "pt_init")
    r = capi.Renderer(scene, pixel_begin=10, pixel_count=W * 3)
    try:
        before = r.stats().device_bytes
        # the flag word: the new bit only beside the moments, and the filter's word keeps refusing it
        for name, call in (("pt_history_reproject_ex", lambda fl: L.pt_history_reproject_ex(None, fl)), ("pt_history_capture_ex", lambda fl: L.pt_history_capture_ex(C.c_float(-1.0), fl))):
            refused(call(FB), name, "PT_HISTORY_FEEDBACK needs PT_HISTORY_MOMENTS")
            refused(call(FB | VAR), name, "PT_HISTORY_FEEDBACK", "not with PT_HISTORY_VARIANCE")
            refused(call(FB | VAR | MOM), name, "exclude each other")
            refused(call(FB | MOM | 8), name, "undefined flag bit(s) 0x8")
            refused(call(FB | MOM), name, "whole contiguous image rows")  # accepted by the flag check
        refused(L.pt_history_reproject_ex(None, FB | MOTION), "pt_history_reproject_ex", "needs PT_HISTORY_MOMENTS")
        refused(L.pt_history_capture_ex(C.c_float(-1.0), FB | MOM | MOTION), "pt_history_capture_ex", "undefined flag bit(s) 0x4")
        refused(L.pt_history_denoise_ex(C.c_float(-1.0), None, MOM | FB, None), "pt_history_denoise_ex", "undefined flag bit(s) 0x10")
        refused(L.pt_history_denoise_feedback(C.c_float(-1.0), None, fbo(9), None), who, "whole contiguous image rows")
        assert r.stats().device_bytes == before
    finally:
        r.free()
    r = capi.Renderer(scene)
    try:
        before = r.stats().device_bytes
        bad_dn = C.byref(capi.PtDenoiseOptions(9, 0.0, 0.0, 0.0, 0))
        bad_hi = C.byref(capi.PtHistoryOptions(-1.0, 0.0, 0.0, 0))
        refused(L.pt_history_denoise_feedback(C.c_float(-1.0), bad_dn, fbo(9), None), who, "no feature pass")
        assert r.stats().device_bytes == before
        r.render(1, 1)
        r.render_features(1, 1)
        before = r.stats().device_bytes
        # the moments form's refusals first, in their order; then fb; then the null buffer
        refused(L.pt_history_denoise_feedback(C.c_float(-1.0), bad_dn, fbo(9), None), who, "samples")
        refused(L.pt_history_denoise_feedback(one, bad_dn, fbo(9), None), who, "levels")
        refused(L.pt_history_denoise_feedback(one, C.byref(capi.PtDenoiseOptions(0, 0.0, 0.0, 0.0, 2)), fbo(9), None), who, "keep_albedo")
        refused(L.pt_history_denoise_feedback(one, None, fbo(6), None), who, "feedback level 6 is not in 1 .. 5")
        refused(L.pt_history_denoise_feedback(one, C.byref(capi.PtDenoiseOptions(2, 0.0, 0.0, 0.0, 0)), fbo(3), None), who, "feedback level 3 is not in 1 .. 2")
        refused(L.pt_history_denoise_feedback(one, None, fbo(-1), None), who, "feedback level -1")
        refused(L.pt_history_denoise_feedback(one, None, fbo(0, 2), None), who, "feedback variance 2")
        refused(L.pt_history_denoise_feedback(one, None, fbo(6, 2), None), who, "feedback level 6")
        refused(L.pt_history_denoise_feedback(one, None, None, None), who, "null")
        # the capture: P absent comes after what the capture refused before
        refused(L.pt_history_capture_ex(C.c_float(-1.0), MOM | FB), "pt_history_capture_ex", "samples")
        refused(L.pt_history_capture_ex(one, MOM | FB), "pt_history_capture_ex", "the pending plane is absent", "pt_history_denoise_feedback")
        assert r.stats().device_bytes == before  # nothing allocated by any of them
        # the lookup: nothing captured with feedback comes after the options and after "with moments"
        r.history_capture(SPP)
        refused(L.pt_history_reproject_ex(bad_hi, MOM | FB), "pt_history_reproject_ex", "cap")
        refused(L.pt_history_reproject_ex(None, MOM | FB), "pt_history_reproject_ex", "nothing has been captured with moments")
        r.history_capture_ex(SPP, MOM)
        refused(L.pt_history_reproject_ex(bad_hi, MOM | FB), "pt_history_reproject_ex", "cap")
        refused(L.pt_history_reproject_ex(None, MOM | FB), "pt_history_reproject_ex", "nothing has been captured with feedback", "PT_HISTORY_FEEDBACK")
        refused(L.pt_history_reproject_ex(None, MOM | FB | MOTION), "pt_history_reproject_ex", "nothing has been captured with feedback")
        # C present with FC absent: after fb, before the null buffer; C of another kind before both
        r.history_reproject()
        refused(L.pt_history_denoise_feedback(one, None, fbo(6), None), who, "the current plane has no moments")
        refused(L.pt_history_capture_ex(one, MOM | FB), "pt_history_capture_ex", "the current plane has no moments")
        r.history_reproject_ex(MOM)
        refused(L.pt_history_denoise_feedback(one, None, fbo(6), None), who, "feedback level 6")
        refused(L.pt_history_denoise_feedback(one, None, fbo(1), None), who, "the current plane has no filtered colour", "PT_HISTORY_FEEDBACK")
        refused(L.pt_history_denoise_feedback(one, None, fbo(1), p), who, "the current plane has no filtered colour")
        assert r.stats().device_bytes == before + 64 * N + 32 * N + 16  # K and C, VK and VC, reject_geom: nothing for the feedback
        # rule 1 in another unit than the carried variance's: only while FC is present, after "C without FC", before the null buffer
        r.clear(), one_view(r)
        keep = C.byref(capi.PtDenoiseOptions(0, 0.0, 0.0, 0.0, 1))
        assert L.pt_history_denoise_feedback(one, keep, fbo(1, 1), p) == 0  # FC absent: any keep_albedo
        r.history_capture_ex(SPP, MOM | FB)
        assert L.pt_history_denoise_feedback(one, None, fbo(1, 1), p) == 0  # FC still absent
        r.history_reproject_ex(MOM)
        refused(L.pt_history_denoise_feedback(one, None, fbo(1, 1), None), who, "the current plane has no filtered colour")
        r.history_reproject_ex(MOM | FB)
        refused(L.pt_history_denoise_feedback(one, keep, fbo(1, 1), None), who, "feedback variance 1 with keep_albedo 1", "tapped with keep_albedo 0")
        refused(L.pt_history_denoise_feedback(one, keep, fbo(6, 1), None), who, "feedback level 6")
        refused(L.pt_history_denoise_feedback(one, keep, fbo(1, 0), None), who, "keep_albedo 1")  # the default rule is rule 1
        refused(L.pt_history_denoise_feedback(one, None, fbo(1, 1), None), who, "null")
        assert L.pt_history_denoise_feedback(one, keep, fbo(1, -1), p) == 0  # rule 0 reads no carried variance
        # the adaptive state
        r.clear()
        for g in range(2):
            r.render(g * 4 + 1, 4)
            r.noise_fold()
        r.render_features(1, 1)
        r.adaptive_round(9, 4, 0.25)
        refused(L.pt_history_denoise_feedback(C.c_float(-1.0), bad_dn, fbo(9), p), who, "adaptive state")
        refused(L.pt_history_reproject_ex(bad_hi, MOM | FB), "pt_history_reproject_ex", "adaptive state")
        refused(L.pt_history_capture_ex(C.c_float(-1.0), MOM | FB), "pt_history_capture_ex", "adaptive state")
    finally:
        r.free()
