"""The host twin of the device grid build (pt_camera_grid_host: pt::build_grid forced at a given resolution, the guard cells and copies
camera_tables() adds, the decisions of the device build) against the numpy restatement tests/camera_grid_ref.py, byte for byte, on
synthetic leaves: grids of one cell up to 2^22 cells, the scan's block and pass edges, ranges of thousands of cells, the limits on a
cell's list, on the references and on the cells.  tests/test_gpu_camera_grid.py compares the kernels with this twin.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import camera_grid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "csrc")
CASES = [(name, ch) for name in ref.case_names() for ch in ref.center_halves(name)]
CASE_IDS = ["%s-ch%d" % (ref.case_id(name), ch) for name, ch in CASES]


def host(name, ch):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    nodes, types, _ = ref.case(name)
    res = name[1]
    return capi.camera_grid(nodes, types, np.zeros(3, np.float32), np.asarray(res, np.float32), res, center_half=bool(ch))


def check_result(out, want, res):
    """The scalars of a PtCameraGridResult against the restatement's."""
    origin, cs, inv_cs, pad = ref.shape_words(res)
    assert out.status == want["status"]
    assert (tuple(out.res), out.num_cells, out.guard) == (tuple(res), want["ncell"], want["guard"])
    assert (out.refs, out.longest) == (want["refs"], want["longest"])
    got = np.asarray(list(out.origin) + list(out.cell_size) + list(out.inv_cell_size) + [out.pad], np.float32)
    assert got.tobytes() == np.concatenate([origin, cs, inv_cs, [pad]]).astype(np.float32).tobytes()


@pytest.mark.parametrize("name,ch", CASES, ids=CASE_IDS)
def test_host_grid_equals_the_restatement(name, ch):
    nodes, types, _ = ref.case(name)
    res = name[1]
    want = ref.restate(nodes, types, res, bool(ch))
    out, start, items, items_b = host(name, ch)
    check_result(out, want, res)
    if want["status"] != ref.BUILT:
        assert start is None and items is None and items_b is None
        return
    message = ref.first_difference(start, want["start"], want["guard"], "start")
    assert message is None, message
    message = ref.first_record_difference(items, want["items"], want["start"], want["guard"], "items")
    assert message is None, message
    if ch:
        message = ref.first_record_difference(items_b, want["items_b"], want["start"], want["guard"], "items_b")
        assert message is None, message
    else:
        assert items_b is None


def test_the_grids_reach_the_blocks_and_passes_they_are_there_for():
    for res, (cells, blocks, passes) in ref.GRIDS.items():
        assert res[0] * res[1] * res[2] == cells
        assert ref.blocks_and_passes(cells) == (blocks, passes), res
    assert ref.GRIDS[ref.WHOLE][0] == ref.MAX_CELLS and ref.TOO_MANY_CELLS[0] * ref.TOO_MANY_CELLS[1] * ref.TOO_MANY_CELLS[2] > ref.MAX_CELLS
    assert 286639 - 279 * 1024 == 943 and 286639 % 4 == 3 and 105 % 4 == 1  # a short last block; the per-thread tails
    assert ref.blocks_and_passes(ref.CROWDED_CELL + 1) == (257, 2) and ref.CROWDED_CELL % (ref.PER_BLOCK * ref.PER_PASS) == 0
    for name in ref.case_names():  # every case was given its grid's population
        if name[0] == "per_block" and name[1] in ref.GRIDS:
            cells = ref.per_block_cells(name[1])
            counts = np.bincount(cells // ref.PER_BLOCK)
            assert counts.size == ref.GRIDS[name[1]][1] and counts.min() >= 1 and cells[-1] == ref.GRIDS[name[1]][0] - 1
            if counts.size > 3:
                assert set(counts[:-1]) == {1, 2, 3}


def cells_of(nodes, leaves, res):
    c0, c1 = ref.cell_range(nodes["bmin"][leaves], nodes["bmax"][leaves], res)
    return c0, c1, c0[:, 0] + res[0] * (c0[:, 1] + res[1] * c0[:, 2])


@pytest.mark.parametrize("name", ref.case_names(), ids=[ref.case_id(n) for n in ref.case_names()])
def test_every_tiny_leaf_lies_in_its_one_cell(name):
    kind, res = name
    nodes, types, leaves = ref.case(name)
    assert not np.array_equal(leaves, np.arange(leaves.size))  # node index != leaf number
    geoms = nodes["geom"][leaves]
    assert sorted(geoms) == list(range(leaves.size)) and (leaves.size < 3 or not np.array_equal(geoms, np.arange(leaves.size)))
    assert (nodes["geom"][np.setdiff1d(np.arange(nodes.size), leaves)] == -1).all() and nodes.size > leaves.size
    if leaves.size >= 3:
        assert set(types[geoms]) == {0, 1, 2}
    if kind == "per_block":
        tiny, want = leaves, ref.per_block_cells(res)
    elif kind == "slabs":
        tiny, want = leaves[3:], ref.per_block_cells(res)
    elif kind.startswith("crowded"):
        tiny, want = leaves, np.full(leaves.size, ref.CROWDED_CELL if kind == "crowded_4096" else 52)
        assert len({nodes["bmin"][i].tobytes() for i in leaves}) == leaves.size  # the records can be told apart
        assert len(set(np.diff(leaves))) > 1  # no regular stride between the node indices
    elif kind == "whole_1_and_tiny":
        tiny, want = leaves[1:], np.asarray([5])
    else:
        return
    c0, c1, cell = cells_of(nodes, tiny, res)
    assert (c0 == c1).all() and np.array_equal(cell, want)


def test_the_wide_leaves_cover_what_they_are_there_for():
    for res in ref.SLAB_GRIDS:
        nodes, _, leaves = ref.case(("slabs", res))
        c0, c1, _ = cells_of(nodes, leaves[:3], res)
        n = c1 - c0 + 1
        assert tuple(n[0]) == (res[0], res[1], 1) and tuple(n[1]) == (1, 1, res[2]) and tuple(n[2]) == tuple(res)
    for res in ref.RANDOM_GRIDS:  # clamped boxes, boxes wholly outside, faces within an ulp of a cell boundary
        nodes, _, leaves = ref.case(("random", res))
        r = np.asarray(res, np.float32)
        lo, hi = nodes["bmin"][leaves], nodes["bmax"][leaves]
        assert ((hi < 0) | (lo > r)).any() and (((lo < 0) & (hi > 0)) | ((lo < r) & (hi > r))).any()
        pad, flo, ext = ref.frame(res)
        q = ((lo.astype(np.float64) - pad) - flo) / ext * np.asarray(res, np.float64)
        assert (np.abs(q - np.round(q)) < 1e-5).sum() > 1000


def test_host_refusals():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    L = capi.lib()
    nodes, types, _ = ref.case(("per_block", (3, 5, 7)))
    lo, hi, res = np.zeros(3, np.float32), np.asarray([3, 5, 7], np.float32), np.asarray([3, 5, 7], np.int32)
    out = capi.PtCameraGridResult()
    start, items = np.zeros(1000, np.uint32), np.zeros((100, 8), np.uint32)

    def call(nodes=nodes, n=None, types=types, ng=None, lo=lo, hi=hi, mag=0.0, res=res, ch=0, out=out, start=start, items=items, items_b=None, caps=(1000, 100)):
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        return L.pt_camera_grid_host(p(nodes), nodes.size if n is None else n, None if types is None else capi._i(types), types.size if ng is None else ng,
                                     None if lo is None else capi._f(lo), None if hi is None else capi._f(hi), mag, None if res is None else capi._i(res), ch,
                                     None if out is None else C.byref(out), p(start), caps[0], p(items), p(items_b), caps[1])

    assert call() == 0 and out.status == 0
    for kw in (dict(types=None, ng=types.size), dict(lo=None), dict(hi=None), dict(res=None), dict(out=None), dict(start=None), dict(items=None), dict(ch=1),
               dict(n=0), dict(ng=0), dict(mag=-1.0), dict(mag=float("nan")), dict(mag=float("inf")), dict(caps=((3 * 5 + 3 + 2) * 2 + 105, 100)),
               dict(caps=(1000, int(out.refs) - 1))):
        assert call(**kw) != 0, kw
        assert b"pt_camera_grid_host" in L.pt_last_error(), kw
    for field, index, value in (("geom", 1, types.size), ("geom", 1, -2), ("bmin", 1, np.float32("nan")), ("bmax", 1, np.float32("nan")), ("bmin", 1, 100.0)):
        bad = nodes.copy()
        if field == "geom":
            bad[field][index] = value
        else:
            bad[field][index][1] = value
        assert call(nodes=bad) != 0 and b"pt_camera_grid_host" in L.pt_last_error(), (field, value)
    assert call(start=None, items=None, caps=(0, 0)) == 0 and out.status == 0 and out.refs > 0  # the query for the sizes
    flat = call(hi=np.zeros(3, np.float32))  # no extent: no frame, no grid
    assert flat == 0 and out.status == ref.NONE and out.num_cells == 0
    only_inner = nodes.copy()
    only_inner["geom"] = -1
    assert call(nodes=only_inner) == 0 and (out.status, out.refs, out.longest) == (ref.NONE, 0, 0)


def test_host_code_under_the_sanitizers(tmp_path):
    """csrc/pt_tables.cpp and pt_scene.cpp are plain C++: a stand-alone driver (tests/integration/camera_grid_driver.cpp) runs the host
    twin on the small grids and on 257 x 32 x 32 with address and undefined-behaviour checks, built by the system compiler and run
    directly."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no system C++ compiler")
    exe = str(tmp_path / "camera_grid_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
           "-I", CSRC, os.path.join(ROOT, "tests", "integration", "camera_grid_driver.cpp"), os.path.join(CSRC, "pt_tables.cpp"), os.path.join(CSRC, "pt_scene.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr and "camera grid: 33 cases" in r.stdout, (r.returncode, r.stdout, r.stderr)
