"""Write-outs of different widths on ONE group, one after the other (csrc/pt_group.cpp: gather(), PtGroup::d_recv): every payload's
tiles meet in the same receive buffer on the root, and nothing but the order of the root's stream lies between the placement that
reads one payload and the exchange that writes the next.  Each result equals, bit for bit, what one Renderer gives after the same calls.
Several contexts on device 0 (COPY transport), batches of 3 iterations, as tests/test_gpu_group_adaptive.py; the arithmetic modes are
that file's business."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = 3
CAP_FRACTION = 0.25


def visible_devices():
    import torch
    return torch.cuda.device_count()


def same(got, want, what):
    if isinstance(want, dict):
        assert got.keys() == want.keys(), what
        for k in want:
            same(got[k], want[k], (what, k))
    elif not isinstance(want, np.ndarray):  # None, or a round's (above, selected)
        assert got == want, (what, got, want)
    else:
        assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
        a, b = (np.ascontiguousarray(x).reshape(-1).view(np.uint8) for x in (got, want))
        bad = np.flatnonzero(a != b) // got.itemsize
        assert bad.size == 0, (what, bad.size, bad[:8])


def test_widths_follow_each_other_on_uneven_tiles(scene_dir):
    """33 x 7 on three contexts: rows 3/2/2, so the second and third tile start at pixel 0 and 66 of the receive buffer and, for the
    3-byte payload, at odd byte offsets.  4 B, 16 B x planes, 3 B, 12 B, then 4 B and 12 B again."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    scene = capi.Scene(scene_dir["cornell"], res=(33, 7))
    spp = 4

    def rendered(x):
        x.render(1, spp)
        x.render_features(1, 2)

    r = capi.Renderer(scene, iters_per_batch=G)
    try:
        rendered(r)
        want = dict(preview=r.preview(spp), features=r.readback_features(), u8=r.save_u8(float(spp)), image=r.readback())
    finally:
        r.free()
    g = capi.Group(scene, [0, 0, 0], transport="copy", iters_per_batch=G)
    try:
        rendered(g)
        for k, (name, call) in enumerate((("preview", lambda: g.preview(spp)), ("features", g.gather_features), ("u8", lambda: g.gather_u8(float(spp))),
                                          ("image", g.gather), ("preview", lambda: g.preview(spp)), ("image", g.gather))):
            same(call(), want[name], (k, name))
    finally:
        g.free()


def adaptive_frame(scene_dir, devices, **group_kw):
    """97 x 61 (tests/test_gpu_group_adaptive.py: rows 21/20/20 on three contexts), two uniform groups, one round whose list the cap cuts,
    then the write-outs of the adaptive state; pt_group_denoise_adaptive queues the 12, 16 (x 5 planes) and 8 byte exchanges back to back
    without a host synchronise between them.  The contexts' device_bytes moves only where a context's own buffer is first used: the
    group's buffers, the receive buffer among them, are not the contexts'.

    pt_save_u8 refuses the adaptive state, a context's and hence a group's alike: the 3-byte write-out runs before the round, between
    the 16- and 8-byte ones, and after the filter both forms give the same refusal."""
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    res = (97, 61)
    scene = capi.Scene(scene_dir["cornell"], res=res)
    n = len(devices)
    r = capi.Renderer(scene, iters_per_batch=G)
    g = capi.Group(scene, devices, iters_per_batch=G, **group_kw)
    try:
        def context_bytes():
            return sum(g.stats(i).device_bytes for i in range(n))

        def step(what, grows, group_call, single_call):
            """The call on both: the group's result equals the renderer's, and the contexts' memory grows exactly where it is said to."""
            before = context_bytes()
            got = group_call()
            after = context_bytes()
            assert (after > before) if grows else (after == before), (what, before, after)
            same(got, single_call(), what)
            return got

        for j in range(2):
            step(("render", j), False, lambda: g.render(1 + j * G, G), lambda: r.render(1 + j * G, G))
            step(("fold", j), j == 0, g.noise_fold, r.noise_fold)  # the noise planes
        step("render_features", True, lambda: g.render_features(1, 2), lambda: r.render_features(1, 2))
        step("u8 before the round", True, lambda: g.gather_u8(2.0 * G), lambda: r.save_u8(2.0 * G))  # every context's converted bytes
        round_args = (1 + 2 * G, G, 0.0, CAP_FRACTION)
        above, m = step("round", True, lambda: g.adaptive_round_threshold(*round_args), lambda: r.adaptive_round_threshold(*round_args))  # counts, list, worker
        assert above > m > 0, (above, m)
        step("counts", False, g.gather_adaptive, r.readback_adaptive)
        step("resolve", True, g.resolve, r.resolve)  # every context's resolved tile
        step("features", False, g.gather_features, r.readback_features)
        step("denoise_adaptive", False, g.denoise_adaptive, r.denoise_adaptive)
        before, refusals = context_bytes(), []
        for call in (lambda: g.gather_u8(3.0 * G), lambda: r.save_u8(3.0 * G)):
            with pytest.raises(capi.PtError, match="pt_save_u8: .*adaptive state") as e:
                call()
            refusals.append(str(e.value))
        assert refusals[0] == refusals[1] and context_bytes() == before, refusals
        step("image", False, g.gather, r.readback)
        step("counts again", False, g.gather_adaptive, r.readback_adaptive)
    finally:
        g.free()
        r.free()


def test_widths_follow_each_other_around_an_adaptive_round(scene_dir):
    adaptive_frame(scene_dir, [0, 0, 0], transport="copy")


def test_widths_follow_each_other_on_every_visible_device(scene_dir):
    """The same over RCCL: ncclRecv in place of the copies into the receive buffer."""
    ndev = visible_devices()
    if ndev < 2:
        pytest.skip("one visible device: the RCCL exchanges need two")
    adaptive_frame(scene_dir, list(range(ndev)))
