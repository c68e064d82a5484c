"""Cutting a frame's pixel list into the lists of a group's contexts on the host (pt_group_partition_host; csrc/pt_group_select.h)
against the numpy restatement tests/group_select_ref.py, and the properties a group's round relies on: ascending, disjoint parts
that map back to the input through the stripe formula.  No GPU."""
import numpy as np
import pytest

import group_select_ref as gref


def check_parts(what, lst, parts, counts, w, h, n):
    want_parts, want_counts = gref.partition(lst, w, n)
    assert np.array_equal(counts, want_counts) and int(counts.sum()) == lst.size, (what, counts, want_counts)
    back = []
    for i, (got, want) in enumerate(zip(parts, want_parts)):
        assert got.dtype == np.int32 and np.array_equal(got, want), (what, i, got[:8], want[:8])
        assert (np.diff(got) > 0).all(), (what, i)  # ascending tile order, no entry twice
        rows_i = (h - i + n - 1) // n
        assert got.size == 0 or (0 <= got[0] and got[-1] < rows_i * w), (what, i, rows_i)
        back.append(gref.frame_pixels(got, i, w, n))
    back = np.concatenate(back) if back else np.zeros(0, np.int64)
    assert np.unique(back).size == back.size, what  # disjoint
    assert np.array_equal(np.sort(back), lst.astype(np.int64)), what  # ... and together the input list


@pytest.mark.parametrize("w, h, n", gref.SHAPES)
def test_partition_equals_restatement(w, h, n):
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    names = []
    for name, lst in gref.cases(w, h, n):
        parts, counts = capi.group_partition_host(lst, w, h, n)
        check_parts((w, h, n, name), lst, parts, counts, w, h, n)
        names.append(name)
        if name.startswith("only context") and n > 1:
            assert np.count_nonzero(counts) == 1, (name, counts)
    assert {"empty", "first pixel", "every pixel", "only context 0"} <= set(names)
    if w * h > gref.BLOCK:  # longer than one workgroup of the kernel handles, with a ragged last one
        assert any(lst.size > gref.BLOCK and lst.size % gref.BLOCK for _, lst in gref.cases(w, h, n))


def test_partition_refuses():
    from cosc_4397_pathtracing_raytracing_project_amd import capi
    ok = np.array([0, 5, 6], np.int32)
    for lst, w, h, n, match in ((ok, 7, 5, 0, "contexts"), (ok, 7, 5, 6, "contexts"), (ok, 7, 70, 65, "contexts"), (ok, 0, 5, 2, "frame"),
                                (np.array([0, 5, 5], np.int32), 7, 5, 2, r"list\[2\] = 5"), (np.array([3, 2], np.int32), 7, 5, 2, r"list\[1\] = 2"),
                                (np.array([-1], np.int32), 7, 5, 2, r"list\[0\] = -1"), (np.array([35], np.int32), 7, 5, 2, r"list\[0\] = 35"),
                                (np.arange(36, dtype=np.int32), 7, 5, 2, "a list of 36")):
        with pytest.raises(capi.PtError, match="pt_group_partition_host: .*" + match):
            capi.group_partition_host(lst, w, h, n)
