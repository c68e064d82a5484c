"""The centre / half-extent form of the traversal boxes the fast build's bounce kernels test (pt_center_half_box,
csrc/pt_tables.cpp center_half_box; csrc/pt_arith.inc slab_t): the converted box must CONTAIN the min / max box it came from
(a ray that passes the reference's box must not be lost to rounding of the conversion), inner boxes must be larger still,
and both must stay tight.  Host-only."""
import ctypes as C

import numpy as np

from cosc_4397_pathtracing_raytracing_project_amd import capi


def convert(lo, hi, inner):
    L = capi.lib()
    c, h = np.zeros(3, np.float32), np.zeros(3, np.float32)
    lo32, hi32 = np.ascontiguousarray(lo, np.float32), np.ascontiguousarray(hi, np.float32)
    fp = C.POINTER(C.c_float)
    L.pt_center_half_box(lo32.ctypes.data_as(fp), hi32.ctypes.data_as(fp), int(inner), c.ctypes.data_as(fp), h.ctypes.data_as(fp))
    return c, h


def test_converted_boxes_contain_the_original_and_stay_tight():
    rs = np.random.RandomState(3)
    for trial in range(4000):
        scale = 10.0 ** rs.uniform(-3, 5)
        centre = rs.uniform(-1, 1, 3) * 10.0 ** rs.uniform(-2, 5)
        ext = np.abs(rs.normal(size=3)) * scale * (rs.rand(3) > 0.1)  # some axes degenerate (lo == hi)
        lo, hi = (centre - ext).astype(np.float32), (centre + ext).astype(np.float32)
        lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
        c, h = convert(lo, hi, False)
        ci, hi_in = convert(lo, hi, True)
        lo64, hi64, c64, h64 = lo.astype(np.float64), hi.astype(np.float64), c.astype(np.float64), h.astype(np.float64)
        assert (c64 - h64 <= lo64).all() and (c64 + h64 >= hi64).all(), (lo, hi, c, h)
        # tight: at most a few ulps of the coordinates beyond the original box
        slack = 4 * np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)).astype(np.float64) + 1e-37
        assert (lo64 - (c64 - h64) <= slack).all() and ((c64 + h64) - hi64 <= slack).all(), (lo, hi, c, h)
        # inner boxes: the same centre, a half extent larger by >= 1e-5 of the extent and of the coordinates, and not by much more
        assert np.array_equal(c, ci)
        grow = hi_in.astype(np.float64) - h64
        want = 1e-5 * h64 + 1e-5 * np.maximum(np.abs(lo64), np.abs(hi64))
        assert (grow >= 0.99 * want).all() and (grow <= 1.01 * want + slack).all(), (lo, hi, h, hi_in)


def test_special_boxes():
    c, h = convert([0, 0, 0], [0, 0, 0], False)
    assert (c == 0).all() and (h >= 0).all() and (h < 1e-30).all()
    c, h = convert([-3e38, -1, 5], [3e38, 1, 5], False)  # the sum of the faces overflows float: the conversion works in double
    assert np.isfinite(c).all() and np.isfinite(h).all() and c[0] == 0 and h[0] >= 3e38
