// pt_camera_tables.h — the per-element arithmetic of the camera-dependent scene tables (pt_tables.h camera_tables), ONE implementation.
//
// What follows the camera position in the tables is a few ten thousand independent box computations and one counting sort.  The
// functions below are what the host build (pt_tables.cpp: pt_init, pt_set_camera) and the device build (pt_camera_tables.hip:
// pt_set_camera_ex with PT_SET_CAMERA_DEVICE_TABLES) both run per node, per top entry and per (leaf, cell) reference, so that the two
// cannot disagree: the device's tables are the host's byte for byte (tests/test_gpu_camera_tables_device.py), and
// pt_selfcheck_camera_math runs every function here on both sides over edge values and random operands.
//
// Everything is double precision arithmetic on float inputs, each operation a separate IEEE operation (`#pragma clang fp
// contract(off)`; the translation units that include this are built with -ffp-contract=off as well).  What the C++ library would
// supply on the host has a form here that compiles for the device and gives libm's bits:
//   * next_up / next_down: nextafterf(x, +-INFINITY) on the bit pattern — -0 and +0 step to the smallest denormal of the direction's
//     sign (or to -0 / +0 from the other side's smallest denormal), the largest finite value steps to infinity, infinity in the
//     direction stays, a NaN stays a NaN;
//   * finite(): the exponent field, for float and double;
//   * mx / mn: std::max / std::min's comparison (the first argument wins a tie or an unordered pair);
//   * sqrt64 and div64: the compiler's correctly rounded double sqrt and quotient.  For gfx950 they lower to the refined sequences
//     (v_rsq_f64 or v_rcp_f64 with FMA steps and the fix-up instructions); pt_selfcheck_camera_math kinds 0 and 1 check on the
//     device that they round as the host's do.
// Plain C++ apart from PT_HD.
#pragma once
#include <cfloat>
#include <cstdint>
#include <cstring>

#include "pt_portable_math.h"

namespace ptct {

// What the device build declines, so that the host build runs instead (PtSetCameraTimes.fallback names the limit; the tables are the same):
constexpr uint32_t kDeviceMaxList = 4096;        // records in one cell: the ordering pass compares every pair of a cell's records.  The
                                                 // host refuses longer lists itself unless the grid is forced (debug_flags 256)
constexpr int64_t kDeviceMaxCells = 1ll << 22;   // cells: what the scan's workspace is planned for (one word per cell, 4096 block sums)
constexpr int64_t kMaxRefs = 1ll << 22;          // build_grid's own limit: ring entries hold 22-bit record indices

PT_HD uint32_t bits_of(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}
PT_HD float float_of(uint32_t u) {
  float x;
  memcpy(&x, &u, 4);
  return x;
}
PT_HD bool finite(float x) { return (bits_of(x) & 0x7f800000u) != 0x7f800000u; }
PT_HD bool finite(double x) {
  uint64_t u;
  memcpy(&u, &x, 8);
  return (u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
PT_HD double mx(double a, double b) { return a < b ? b : a; }
PT_HD double mn(double a, double b) { return b < a ? b : a; }
PT_HD float mx(float a, float b) { return a < b ? b : a; }
PT_HD float mn(float a, float b) { return b < a ? b : a; }
PT_HD int mx(int a, int b) { return a < b ? b : a; }
PT_HD int mn(int a, int b) { return b < a ? b : a; }
PT_HD double sqrt64(double x) { return __builtin_sqrt(x); }
PT_HD double div64(double a, double b) { return a / b; }

PT_HD float next_up(float x) {  // nextafterf(x, +INFINITY)
  const uint32_t u = bits_of(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return x + x;  // NaN (quiet, as libm's x + y)
  if (u == 0x7f800000u) return x;                     // +infinity
  if ((u & 0x7fffffffu) == 0u) return float_of(1u);   // +-0: the smallest positive denormal
  return float_of((u >> 31) ? u - 1u : u + 1u);
}
PT_HD float next_down(float x) {  // nextafterf(x, -INFINITY)
  const uint32_t u = bits_of(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return x + x;
  if (u == 0xff800000u) return x;
  if ((u & 0x7fffffffu) == 0u) return float_of(0x80000001u);
  return float_of((u >> 31) ? u + 1u : u - 1u);
}

// Tighter leaf boxes for spheres (the derivation: pt_tables.cpp, tighten_sphere_leaves).  inv: the geom's inverse transform, column-major
// 4x4 (PtGeom.inverseTransform); origin_lo / origin_hi: the region ray origins come from (pt::origin_region); ref_lo / ref_hi: the
// reference's leaf box.  Returns false when nothing could be tightened (lo / hi are then not to be used).
PT_HD bool sphere_tight_box(const float* inv, const double origin_lo[3], const double origin_hi[3], const float ref_lo[3], const float ref_hi[3],
                            float lo[3], float hi[3]) {
#pragma clang fp contract(off)
  const double u = 1.0 / 16777216.0;
  double M = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) M = mx(mx(M, __builtin_fabs(origin_lo[a])), __builtin_fabs(origin_hi[a]));
  M *= sqrt64(3.0);
  double A[3][3], t[3], B[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) A[r][c] = inv[c * 4 + r];
    t[r] = inv[3 * 4 + r];
  }
  const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                     A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
  if (!(__builtin_fabs(det) > 0.0) || !finite(det)) return false;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;  // B = A^-1: cofactor of A[c][r] over det
      B[r][c] = div64(A[r1][c1] * A[r2][c2] - A[r1][c2] * A[r2][c1], det);
    }
  double nA = 0.0, nB = 0.0, nt = 0.0, ctr[3], D = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) nA += A[r][c] * A[r][c], nB += B[r][c] * B[r][c];
    nt += t[r] * t[r];
    ctr[r] = -(B[r][0] * t[0] + B[r][1] * t[1] + B[r][2] * t[2]);
  }
  nA = sqrt64(nA), nB = sqrt64(nB), nt = sqrt64(nt);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double far = mx(__builtin_fabs(ctr[a] - origin_lo[a]), __builtin_fabs(ctr[a] - origin_hi[a]));
    D += far * far;
  }
  const double D_obj = nA * sqrt64(D), M_obj = nA * M + nt;
  const double rho = sqrt64(0.25 + 4.0 * u * (18.0 * D_obj * D_obj + 14.0 * M_obj + 5.0 * nA * nB * D_obj));
  if (!finite(rho)) return false;
  const double slab = 32.0 * (double)FLT_EPSILON * M;
  bool changed = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double half = rho * sqrt64(B[a][0] * B[a][0] + B[a][1] * B[a][1] + B[a][2] * B[a][2]) + slab;
    lo[a] = next_down((float)(ctr[a] - half));
    hi[a] = next_up((float)(ctr[a] + half));
    if (!finite(lo[a]) || !finite(hi[a])) lo[a] = ref_lo[a], hi[a] = ref_hi[a];
    lo[a] = mx(lo[a], ref_lo[a]), hi[a] = mn(hi[a], ref_hi[a]);
    changed = changed || lo[a] != ref_lo[a] || hi[a] != ref_hi[a];
  }
  return changed && lo[0] < hi[0] && lo[1] < hi[1] && lo[2] < hi[2];
}

// A box as centre and half extent for the fast build's slab test, in place in (bmin, bmax) (the derivation: pt_tables.cpp, center_half_box)
PT_HD void center_half_box(float bmin[3], float bmax[3], bool inner, double magnitude) {
#pragma clang fp contract(off)
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double lo = bmin[a], hi = bmax[a];
    const float c = (float)(0.5 * (lo + hi));
    double h = mx(hi - (double)c, (double)c - lo);
    if (inner) h = h * (1.0 + 1e-5) + 1e-5 * magnitude + 1e-30;
    float hf = (float)h;
    if ((double)hf < h) hf = next_up(hf);
    bmin[a] = c, bmax[a] = hf;
  }
}

// The scalars of a grid that every leaf's cell range is computed from (pt::build_grid computes them on the host for both builds)
struct GridFrame {
  double pad, lo[3], ext[3];
  int res[3];
};
// The cells [c0, c1] per axis that a leaf's box grown by `pad` touches.  The clamp to [0, res - 1] happens on the floored double, so
// that a quotient outside the range of int (no leaf inside the grid's frame has one) is clamped, not converted: the same on both sides.
PT_HD int clamp_cell(double v, int res) { return v >= (double)(res - 1) ? res - 1 : v >= 0.0 ? (int)v : 0; }  // (a NaN: cell 0)
PT_HD void cell_range(const float bmin[3], const float bmax[3], const GridFrame& f, int c0[3], int c1[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    c0[a] = clamp_cell(__builtin_floor(div64((double)bmin[a] - f.pad - f.lo[a], f.ext[a]) * f.res[a]), f.res[a]);
    c1[a] = clamp_cell(__builtin_floor(div64((double)bmax[a] + f.pad - f.lo[a], f.ext[a]) * f.res[a]), f.res[a]);
  }
}
PT_HD int64_t cell_references(const int c0[3], const int c1[3]) { return (int64_t)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1); }
PT_HD size_t cell_index(const int res[3], int x, int y, int z) { return (size_t)x + (size_t)res[0] * ((size_t)y + (size_t)res[1] * z); }
// The `geom` word of the record of a leaf in cell (x, y, z) of its range: bits 0-5 the leaf is also listed in the neighbour cell
// -x, +x, -y, +y, -z, +z; bits 6-7 the primitive's type; bits 8-31 its index
PT_HD int32_t record_geom_word(int x, int y, int z, const int c0[3], const int c1[3], int type, int geom) {
  return (x > c0[0] ? 1 : 0) | (x < c1[0] ? 2 : 0) | (y > c0[1] ? 4 : 0) | (y < c1[1] ? 8 : 0) | (z > c0[2] ? 16 : 0) | (z < c1[2] ? 32 : 0) |
         ((type & 3) << 6) | (geom << 8);
}


// ---- what the device build (pt_camera_tables.hip) and its caller (pt_api.cpp) share --------------------------------------------------
struct DeviceGeom {  // the fields of a PtGeom the build reads
  float inv[16];     // inverseTransform
  int32_t type;
  int32_t pad[3];
};
static_assert(sizeof(DeviceGeom) == 80, "DeviceGeom is 80 B");
struct BuildRecord {  // what the host reads back between the count and the scan
  unsigned long long refs;  // (leaf, cell) references
  uint32_t longest;         // records in the fullest cell (0 when refs exceeds kMaxRefs: nothing was counted)
  uint32_t tight;           // sphere leaves with a tightened box
};
static_assert(sizeof(BuildRecord) == 16, "BuildRecord is 16 B");
struct BuildArgs {
  int32_t num_nodes, num_top;
  int32_t tighten, center_half;  // tighten: kTightNodes nodes or more and not debug_flags 2048
  double origin_lo[3], origin_hi[3], magnitude;
  GridFrame frame;               // the grid launches only
  uint32_t guard, ncell;
};
// Operands and results of pt_selfcheck_camera_math, one set per element
struct MathOp {
  double d[8];
  float f[24];
};
struct MathOut {
  uint32_t w[16];
};
constexpr int kMathKinds = 6;

}  // namespace ptct
