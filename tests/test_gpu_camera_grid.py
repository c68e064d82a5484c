"""The grid kernels of the device build of the camera-dependent tables (csrc/pt_camera_tables.hip: k_ct_refs, k_ct_count, k_ct_longest,
k_ct_block_sums, k_ct_scan_sums, k_ct_scan_write, k_ct_guards, k_ct_scatter, k_ct_records) on synthetic leaves, through
pt_stage_camera_grid, against the host twin pt_camera_grid_host byte for byte: every array, refs, longest, status, shape and guard, on
the cases of tests/camera_grid_ref.py (tests/test_camera_grid_host.py holds the twin to the numpy restatement).  What no scene reaches
in a test: up to 16 passes of k_ct_scan_sums, the block and per-thread tails of the scan, ranges of up to 2^22 cells, the limits on a
cell's list, the references and the cells.  One tiny cornell renderer is the default context; it renders nothing."""
import ctypes as C

import numpy as np
import pytest

import camera_grid_ref as ref
from camera_scenes import cornell_text, scene_path

pytestmark = pytest.mark.gpu
CASES = [(name, ch) for name in ref.case_names() for ch in ref.center_halves(name)]
CASE_IDS = ["%s-ch%d" % (ref.case_id(name), ch) for name, ch in CASES]


@pytest.fixture(scope="module")
def renderer(tmp_path_factory):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    r = capi.Renderer(capi.Scene(scene_path(tmp_path_factory.mktemp("camera_grid"), cornell_text, "A")))
    yield r
    r.free()


def both(name, ch):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    nodes, types, _ = ref.case(name)
    res = name[1]
    lo, hi = np.zeros(3, np.float32), np.asarray(res, np.float32)
    host = capi.camera_grid(nodes, types, lo, hi, res, center_half=bool(ch))
    # the arrays are sized by what the host built: a device build that counts more is refused by the stage, and the test fails
    caps = (host[1].size, host[2].shape[0]) if host[0].status == 0 else (1, 1)
    return host, capi.camera_grid(nodes, types, lo, hi, res, center_half=bool(ch), device=True, caps=caps)


def scalars(out):
    return (out.status, tuple(out.res), out.num_cells, out.guard, out.refs, out.longest,
            np.asarray(list(out.origin) + list(out.cell_size) + list(out.inv_cell_size) + [out.pad], np.float32).tobytes())


@pytest.mark.parametrize("name,ch", CASES, ids=CASE_IDS)
def test_device_grid_equals_host_grid(renderer, name, ch):
    (h_out, h_start, h_items, h_items_b), (d_out, d_start, d_items, d_items_b) = both(name, ch)
    assert scalars(d_out) == scalars(h_out)
    kind, res = name
    ncell = res[0] * res[1] * res[2]
    # what the case is there for
    if res == ref.TOO_MANY_CELLS:
        assert (d_out.status, d_out.refs, d_out.longest) == (ref.CELLS, 0, 0)
    elif kind == "whole_1":
        assert (d_out.status, d_out.refs, d_out.longest) == (ref.BUILT, ref.MAX_REFS, 1) and ncell == ref.MAX_CELLS
    elif kind == "whole_1_and_tiny":
        assert (d_out.status, d_out.refs, d_out.longest) == (ref.NONE, ref.MAX_REFS + 1, 0)
    elif kind == "whole_1100":
        assert (d_out.status, d_out.refs, d_out.longest) == (ref.NONE, 1100 * ref.MAX_REFS, 0) and d_out.refs > 1 << 32
    elif kind == "crowded_4096":
        assert (d_out.status, d_out.refs, d_out.longest) == (ref.BUILT, 4096, 4096)
    elif kind == "crowded_4097":
        assert (d_out.status, d_out.refs, d_out.longest) == (ref.LIST, 4097, 4097)
    elif kind in ("per_block", "slabs"):
        assert d_out.status == ref.BUILT
    if h_out.status != ref.BUILT:
        assert d_start is None and d_items is None
        return
    guard = int(h_out.guard)
    message = ref.first_difference(d_start, h_start, guard, "start (device against host)")
    assert message is None, message
    message = ref.first_record_difference(d_items, h_items, h_start, guard, "items (device against host)")
    assert message is None, message
    if ch:
        message = ref.first_record_difference(d_items_b, h_items_b, h_start, guard, "items_b (device against host)")
        assert message is None, message
    else:
        assert d_items_b is None
    if kind == "crowded_4096":  # the records of the one full cell, in ascending node index
        s = d_start[guard + ref.CROWDED_CELL:guard + ref.CROWDED_CELL + 2].astype(np.int64)
        assert (s[0], s[1]) == (0, 4096) and (np.diff(d_items[:, 6].astype(np.int64)) > 0).all()


def test_stage_refusals(renderer):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    L = capi.lib()
    nodes, types, _ = ref.case(("per_block", (3, 5, 7)))
    lo, hi, res = np.zeros(3, np.float32), np.asarray([3, 5, 7], np.float32), np.asarray([3, 5, 7], np.int32)
    out = capi.PtCameraGridResult()
    start, items = np.zeros(1000, np.uint32), np.zeros((100, 8), np.uint32)

    def call(nodes=nodes, n=None, types=types, ng=None, lo=lo, hi=hi, mag=0.0, res=res, ch=0, out=out, start=start, items=items, items_b=None, caps=(1000, 100)):
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        return L.pt_stage_camera_grid(p(nodes), nodes.size if n is None else n, None if types is None else capi._i(types), types.size if ng is None else ng,
                                      None if lo is None else capi._f(lo), None if hi is None else capi._f(hi), mag, None if res is None else capi._i(res), ch,
                                      None if out is None else C.byref(out), p(start), caps[0], p(items), p(items_b), caps[1])

    assert call() == 0 and out.status == 0
    refs = int(out.refs)
    for kw in (dict(types=None, ng=types.size), dict(lo=None), dict(hi=None), dict(res=None), dict(out=None), dict(start=None), dict(items=None), dict(ch=1),
               dict(n=0), dict(ng=0), dict(mag=-1.0), dict(mag=float("nan")), dict(mag=float("inf")), dict(caps=((3 * 5 + 3 + 2) * 2 + 105, 100)),
               dict(caps=(1000, refs - 1))):
        assert call(**kw) != 0, kw
        assert b"pt_stage_camera_grid" in L.pt_last_error(), kw
    for field, value in (("geom", types.size), ("geom", -2), ("bmin", np.float32("nan")), ("bmax", np.float32("nan")), ("bmin", 100.0)):
        bad = nodes.copy()
        if field == "geom":
            bad[field][1] = value
        else:
            bad[field][1][1] = value
        assert call(nodes=bad) != 0 and b"pt_stage_camera_grid" in L.pt_last_error(), (field, value)
    assert call(start=None, items=None, caps=(0, 0)) == 0 and (out.status, out.refs) == (0, refs)  # the query for the sizes
    assert call(hi=np.zeros(3, np.float32)) == 0 and (out.status, out.num_cells) == (ref.NONE, 0)  # no extent: no frame, nothing launched
    only_inner = nodes.copy()
    only_inner["geom"] = -1
    assert call(nodes=only_inner) == 0 and (out.status, out.refs, out.longest) == (ref.NONE, 0, 0)
    # the renderer's own tables are left alone
    before = renderer.read_tables()
    assert call() == 0
    assert renderer.read_tables() == before
