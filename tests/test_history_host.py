"""The reprojected sample history on the host (pt_history_capture_host / _reproject_host / _blend_host: csrc/pt_history.h, the bodies the
HIP kernels run too) against the numpy restatement tests/history_ref.py, bit for bit.  No GPU."""
import numpy as np
import pytest

import features_ref
import history_ref as ref
from history_ref import bits, f32


def same(got, want, what=""):
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:8], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


@pytest.fixture(scope="module")
def cornell_views(tmp_path_factory):
    """Two views of cornell 96 x 54, 3 degrees apart: (PtCamera, S of 4 iterations, feature planes of one iteration), and reject_geom."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    from oracle import binding as ob
    paths = ref.orbit_scene_paths(tmp_path_factory.mktemp("history_host"), frames=2)
    views = []
    ob.set_math_mode(ob.PORTABLE)
    try:
        for f, path in enumerate(paths):
            feat = ref.pack_features(features_ref.iteration_values(ob, path, ref.RES, False, 1))
            ob.load_scene(path, res=ref.RES)
            S = ob.render(f * ref.SPP + 1, ref.SPP, variant=ob.RETIRE, nthreads=8)
            views.append((capi.Scene(path, res=ref.RES).camera, S, feat))
    finally:
        ob.set_math_mode(ob.LIBM)
    return views, capi.reject_geoms(capi.Scene(paths[0], res=ref.RES))


def test_cornell_two_cameras(cornell_views):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    views, reject = cornell_views
    w, h = ref.RES
    (cam0, S0, feat0), (cam1, S1, feat1) = views
    K = capi.history_capture_host(S0, feat0, ref.SPP)
    same(K, ref.capture(S0, feat0, ref.SPP), "capture, C absent")
    same(K[0, :, :3], S0 / f32(ref.SPP), "the first capture keeps S / samples")
    assert (K[0, :, 3] == ref.SPP).all()
    for name, opts in ref.OPTION_SETS.items():
        C = capi.history_reproject_host(cam0, K, feat1, reject, w, h, **opts)
        same(C, ref.reproject(cam0, K, feat1, reject, w, h, **opts), f"reproject {name}")
    C = capi.history_reproject_host(cam0, K, feat1, reject, w, h)
    carried = C[:, 3] > 0
    hit = feat1[1, :, 3] > 0  # (at 96 x 54 less than half of the frame sees the box)
    print(f"cornell, 3 degrees: {carried.sum()} of {carried.size} pixels carried, {hit.sum()} hit")
    assert not carried[~hit].any() and 0.9 < carried[hit].mean() < 1.0
    same(capi.history_blend_host(S1, ref.SPP, C), ref.blend(S1, ref.SPP, C), "blend")
    K1 = capi.history_capture_host(S1, feat1, ref.SPP, C)
    same(K1, ref.capture(S1, feat1, ref.SPP, C), "capture with C")
    same(K1[0, :, :3], ref.blend(S1, ref.SPP, C), "the capture keeps the blend")
    assert (K1[0, carried, 3] == 2 * ref.SPP).all() and (K1[0, ~carried, 3] == ref.SPP).all()


def test_a_mirror_carries_nothing_unless_asked(cornell_views):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    views, reject = cornell_views
    w, h = ref.RES
    (cam0, S0, feat0), (_, _, feat1) = views
    assert reject.tolist() == [0, 0, 0, 0, 0, 0, 1]  # cornell's sphere is the mirror
    ids = np.ascontiguousarray(feat1[2, :, 3]).view(np.int32)
    mirror = ids == 7
    assert mirror.sum() > 30
    K = capi.history_capture_host(S0, feat0, ref.SPP)
    C = capi.history_reproject_host(cam0, K, feat1, reject, w, h)
    assert not C[mirror].any()
    kept = capi.history_reproject_host(cam0, K, feat1, reject, w, h, keep_view_dependent=True)
    assert (kept[mirror, 3] > 0).mean() > 0.8
    same(kept[~mirror], C[~mirror], "the mask touches the listed geoms only")


@pytest.mark.parametrize("name", sorted(ref.OPTION_SETS))
@pytest.mark.parametrize("row0", ref.ROW0)
@pytest.mark.parametrize("w,rows", ref.SHAPES)
def test_adversarial_arrays(w, rows, row0, name):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    cam, kept, feat, reject, _ = ref.adversarial(w, rows, row0)
    got = capi.history_reproject_host(cam.to_capi(), kept, feat, reject, w, rows, row0, **ref.OPTION_SETS[name])
    want = ref.reproject(cam, kept, feat, reject, w, rows, row0, **ref.OPTION_SETS[name])
    assert np.isfinite(want).all()
    same(got, want, f"{w}x{rows} row0 {row0} {name}")


@pytest.mark.parametrize("row0", ref.ROW0)
@pytest.mark.parametrize("w,rows", [(5, 3), (97, 61)])
def test_adversarial_arrays_hold_what_the_lookup_branches_on(w, rows, row0):
    cam, kept, feat, reject, plant = ref.adversarial(w, rows, row0)
    H = cam.resolution[1]
    st = {}
    C = ref.reproject(cam, kept, feat, reject, w, rows, row0, stats=st, min_normal_dot=-1.0, plane_tol=-1.0, keep_view_dependent=True)
    sx, sy, dz, wsum = st["sx"], st["sy"], st["dz"], st["wsum"]
    assert np.isnan(sx[plant["nan"]]) and not np.isfinite(sy[plant["inf"]])
    assert dz[plant["behind"]] < 0 and dz[plant["dz0"]] == 0 and not st["hit"][plant["miss"]]
    assert sx[plant["left_edge"]] == -1 and sx[plant["right_edge"]] == w - 1 and sy[plant["top_edge"]] == -1 and sy[plant["bottom_edge"]] == H - 1
    assert sx[plant["past_left"]] == -1.25 and sx[plant["past_right"]] == w and sy[plant["past_top"]] == -1.5 and sy[plant["past_bottom"]] == H
    for name in ("nan", "inf", "behind", "dz0", "miss", "past_left", "past_right", "past_top", "past_bottom"):
        assert not C[plant[name]].any(), name
    assert wsum[plant["at_64th"]] == f32(0.015625) and C[plant["at_64th"], 3] > 0
    assert f32(0.015625) - f32(2.0 ** -15) < wsum[plant["under_64th"]] < f32(0.015625) and not C[plant["under_64th"]].any()
    assert wsum[plant["left_edge"]] == 0 and not C[plant["left_edge"]].any()  # fx = -1, ax = 0: the whole weight on the column outside
    assert ((sx == np.floor(sx)) & (sy == np.floor(sy))).sum() > 0  # both coordinates on integers
    assert (kept[0, :, 3] == 0).any()
    # and the options change the outcome: the tilted normals, the off-plane depths, the listed geom, the cap
    base = ref.reproject(cam, kept, feat, reject, w, rows, row0)
    for opts in (dict(min_normal_dot=-1.0), dict(plane_tol=-1.0), dict(keep_view_dependent=True), dict(cap=8.0)):
        if w * rows > 100:
            assert (bits(ref.reproject(cam, kept, feat, reject, w, rows, row0, **opts)) != bits(base)).any(), opts


def test_blend_with_c_absent_is_s_over_samples():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    rng = np.random.default_rng(5)
    S = (rng.random((1000, 3), dtype=f32) * f32(40.0)).astype(f32)
    S[:7] = [[0, 0, 0], [np.inf, 1, 2], [np.nan, 0, 1], [1e-45, 1e-40, 3e38], [1, 2, 3], [0.1, 0.2, 0.3], [7, 7, 7]]
    for samples in (1.0, 3.0, 4.0, 7.5):
        with np.errstate(all="ignore"):
            want = S / f32(samples)
        same(capi.history_blend_host(S, samples), want, f"absent, {samples}")
        same(capi.history_blend_host(S, samples, np.zeros((1000, 4), f32)), want, f"zeros, {samples}")
    C = rng.random((1000, 4), dtype=f32)
    C[:, 3] *= f32(32.0)
    same(capi.history_blend_host(S, 4.0, C), ref.blend(S, 4.0, C), "blend")


def test_capture_of_random_arrays():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    import denoise_ref
    for w, rows in ref.SHAPES:
        rgb, planes = denoise_ref.random_frame(w, rows, 4)
        C = np.random.default_rng(w).random((w * rows, 4), dtype=f32)
        same(capi.history_capture_host(rgb, planes, 4.0, C), ref.capture(rgb, planes, 4.0, C), f"{w}x{rows}")
        same(capi.history_capture_host(rgb, planes, 4.0), ref.capture(rgb, planes, 4.0), f"{w}x{rows} absent")


@pytest.mark.parametrize("bad", [dict(cap=-1.0), dict(cap=float("nan")), dict(cap=float("inf")), dict(min_normal_dot=float("nan")),
                                 dict(plane_tol=float("inf")), dict(plane_tol=float("-inf"))])
def test_options_out_of_range_are_refused(bad):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    cam, kept, feat, reject, _ = ref.adversarial(5, 3, 0)
    with pytest.raises(capi.PtError, match="pt_history_reproject_host"):
        capi.history_reproject_host(cam.to_capi(), kept, feat, reject, 5, 3, 0, **bad)


def test_keep_view_dependent_is_zero_or_one_and_samples_are_positive():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    import ctypes as C
    cam, kept, feat, reject, _ = ref.adversarial(5, 3, 0)
    opt = capi.PtHistoryOptions(0.0, 0.0, 0.0, 2)
    out = np.empty((15, 4), f32)
    rc = capi.lib().pt_history_reproject_host(5, 3, 0, C.byref(cam.to_capi()), capi._f(kept.reshape(-1)), capi._f(feat.reshape(-1)),
                                              reject.ctypes.data_as(C.POINTER(C.c_uint8)), reject.size, C.byref(opt), capi._f(out))
    assert rc != 0 and b"pt_history_reproject_host" in capi.lib().pt_last_error()
    S = np.ones((15, 3), f32)
    for samples in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(capi.PtError, match="pt_history_blend_host"):
            capi.history_blend_host(S, samples)
        with pytest.raises(capi.PtError, match="pt_history_capture_host"):
            capi.history_capture_host(S, feat, samples)


def test_the_tile_must_lie_in_the_kept_frame():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    cam, kept, feat, reject, _ = ref.adversarial(5, 3, 0)
    with pytest.raises(capi.PtError, match="pt_history_reproject_host"):
        capi.history_reproject_host(cam.to_capi(), kept, feat, reject, 5, 3, 4)  # rows 4 .. 6 of a frame of 6
    with pytest.raises(capi.PtError):
        capi.history_reproject_host(cam.to_capi(), kept, feat, reject, 5, 4, 0)  # arrays of another size
