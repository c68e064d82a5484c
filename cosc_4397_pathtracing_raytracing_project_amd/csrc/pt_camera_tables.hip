// pt_camera_tables.hip — the camera-dependent scene tables built on the device (pt_set_camera_ex with PT_SET_CAMERA_DEVICE_TABLES), and
// the device half of pt_selfcheck_camera_math.
//
// A translation unit of its own, compiled ONCE with -ffp-contract=off like pt_noise.hip: the per-element arithmetic is the shared
// header's (pt_camera_tables.h), which pt_tables.cpp runs on the host, so the tables are the host's byte for byte.  The inputs are the
// device copy of pt::CameraBase (the untightened threaded BVH, the base top list, the geoms' inverse transforms and types) and the
// scalars the host computes as ever (origin region, scene magnitude, the grid's frame).  No floating-point atomics; no kernel waits
// for another workgroup; the finished tables depend on nothing but their inputs, whatever order the integer atomics ran in.
//
//   k_ct_nodes       one thread per node: the base node, a sphere leaf tightened, -> nodes; its centre / half extent copy -> nodes_b.
//                    Tightened leaves are counted per wave with ballot + popcount and one integer atomic.
//   k_ct_top         one wave: the base entry, a leaf entry with the box of its (tightened) node, -> top; the copy -> top_b.
//   k_ct_refs        one thread per node: a leaf's cell range and its volume, added up per wave and with one 64-bit integer atomic.
//   k_ct_count       one WAVE per leaf (a wall touches a thousand cells, a small primitive one: the lanes share the range): every cell
//                    of the range gets one more in its counter.  Does nothing when the references exceed build_grid's limit, so the
//                    work of all grid kernels is bounded by it.
//   k_ct_longest     one thread per cell: the fullest cell, a maximum per wave and one integer atomic.
//        -- the host reads BuildRecord (references, longest list, tightened leaves), applies build_grid's refusals, sizes the buffers --
//   k_ct_block_sums, k_ct_scan_sums, k_ct_scan_write   the counters become the cell table `start` behind its front guard cells, in three
//                    launches (a workgroup's 1024 cells, the workgroups' sums in one workgroup, the cells again); the counters return
//                    to zero for the scatter.  k_ct_guards writes the guard cells: 0 in front, the total behind.
//   k_ct_scatter     one wave per leaf: its index into a scratch list at start[c] + atomicAdd(fill[c]) — any order inside a cell.
//   k_ct_records     one wave per leaf: for each cell of its range the leaf's rank among the cell's scratch entries (the number of
//                    smaller indices) says where its record goes: threaded order inside every cell, as build_grid's loop gives it.
//                    Writes the 32-byte record (skip = leaf, the `geom` word) and its centre / half extent copy.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_camera_tables_device.h"
#include "pt_internal.h"

namespace {
using ptct::BuildArgs;
using ptct::BuildRecord;
using ptct::DeviceGeom;
using ptct::MathOp;
using ptct::MathOut;
using ptd::Node;
using ptd::TopEntry;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kPerThread = 4;
constexpr int kPerBlock = kBlock * kPerThread;  // cells of a workgroup in the scan

// 32-byte table entries as two 16-byte words (the tables are hipMalloc'ed: every entry is 16-byte aligned)
template <typename T>
__device__ __forceinline__ T load32(const T* p) {
  static_assert(sizeof(T) == 32, "a 32-byte table entry");
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  T v;
  memcpy(&v, &a, 16);
  memcpy(reinterpret_cast<char*>(&v) + 16, &b, 16);
  return v;
}
template <typename T>
__device__ __forceinline__ void store32(T* p, const T& v) {
  static_assert(sizeof(T) == 32, "a 32-byte table entry");
  uint4 a, b;
  memcpy(&a, &v, 16);
  memcpy(&b, reinterpret_cast<const char*>(&v) + 16, 16);
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = a, q[1] = b;
}

__global__ __launch_bounds__(kBlock) void k_ct_nodes(BuildArgs a, const Node* __restrict__ base, const DeviceGeom* __restrict__ geoms, Node* __restrict__ nodes,
                                                     Node* __restrict__ nodes_b, BuildRecord* __restrict__ rec) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  bool tightened = false;
  if (i < a.num_nodes) {
    Node n = load32(base + i);
    if (a.tighten && n.geom >= 0 && geoms[n.geom].type == PT_GEOM_SPHERE) {
      float lo[3], hi[3];
      if (ptct::sphere_tight_box(geoms[n.geom].inv, a.origin_lo, a.origin_hi, n.bmin, n.bmax, lo, hi)) {
        tightened = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) n.bmin[k] = lo[k], n.bmax[k] = hi[k];
      }
    }
    store32(nodes + i, n);
    if (a.center_half) {
      Node b = n;
      ptct::center_half_box(b.bmin, b.bmax, n.geom < 0, a.magnitude);
      store32(nodes_b + i, b);
    }
  }
  const unsigned long long m = __ballot(tightened);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&rec->tight, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(64) void k_ct_top(BuildArgs a, const TopEntry* __restrict__ base, const Node* __restrict__ nodes, TopEntry* __restrict__ top,
                                               TopEntry* __restrict__ top_b) {
  const int e = (int)threadIdx.x;
  if (e >= a.num_top) return;
  TopEntry t = load32(base + e);
  if (a.tighten && t.link < 0 && t.idx >= 0 && t.idx < a.num_nodes) {
    const Node n = load32(nodes + t.idx);
#pragma unroll
    for (int k = 0; k < 3; ++k) t.bmin[k] = n.bmin[k], t.bmax[k] = n.bmax[k];
  }
  store32(top + e, t);
  if (a.center_half) {
    TopEntry b = t;
    ptct::center_half_box(b.bmin, b.bmax, t.link >= 0, a.magnitude);
    store32(top_b + e, b);
  }
}

__global__ __launch_bounds__(kBlock) void k_ct_refs(BuildArgs a, const Node* __restrict__ nodes, BuildRecord* __restrict__ rec) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  unsigned long long refs = 0ull;
  if (i < a.num_nodes) {
    const Node n = load32(nodes + i);
    if (n.geom >= 0) {
      int c0[3], c1[3];
      ptct::cell_range(n.bmin, n.bmax, a.frame, c0, c1);
      refs = (unsigned long long)ptct::cell_references(c0, c1);
    }
  }
  for (int off = 32; off > 0; off >>= 1) refs += __shfl_down(refs, off, 64);
  if ((threadIdx.x & 63) == 0 && refs) atomicAdd(&rec->refs, refs);
}

// The cells of one leaf's range, dealt to the lanes of the wave that owns the leaf
struct Range {
  int c0[3], c1[3], nx, nxy, total;
  __device__ __forceinline__ Range(const Node& n, const BuildArgs& a) {
    ptct::cell_range(n.bmin, n.bmax, a.frame, c0, c1);
    nx = c1[0] - c0[0] + 1;
    nxy = nx * (c1[1] - c0[1] + 1);
    total = nxy * (c1[2] - c0[2] + 1);  // <= ncell <= kDeviceMaxCells
  }
  __device__ __forceinline__ void cell(int k, int* x, int* y, int* z) const {
    const int zz = k / nxy, r = k - zz * nxy, yy = r / nx;
    *x = c0[0] + (r - yy * nx), *y = c0[1] + yy, *z = c0[2] + zz;
  }
};
// the node of this wave, when it is a leaf
__device__ __forceinline__ bool wave_leaf(const BuildArgs& a, const Node* nodes, int* index, Node* n) {
  const int i = (int)(blockIdx.x * kWaves + (threadIdx.x >> 6));
  if (i >= a.num_nodes) return false;
  *index = i;
  *n = load32(nodes + i);
  return n->geom >= 0;
}

__global__ __launch_bounds__(kBlock) void k_ct_count(BuildArgs a, const Node* __restrict__ nodes, const BuildRecord* __restrict__ rec, uint32_t* __restrict__ count) {
  if (rec->refs > (unsigned long long)ptct::kMaxRefs) return;  // build_grid refuses: nothing to count
  int i;
  Node n;
  if (!wave_leaf(a, nodes, &i, &n)) return;
  const Range r(n, a);
  for (int k = (int)(threadIdx.x & 63); k < r.total; k += 64) {
    int x, y, z;
    r.cell(k, &x, &y, &z);
    const size_t c = ptct::cell_index(a.frame.res, x, y, z);
    if (c < (size_t)a.ncell) atomicAdd(&count[c], 1u);
  }
}

__global__ __launch_bounds__(kBlock) void k_ct_longest(uint32_t ncell, const uint32_t* __restrict__ count, BuildRecord* __restrict__ rec) {
  const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
  uint32_t v = c < ncell ? count[c] : 0u;
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = __shfl_down(v, off, 64);
    v = o > v ? o : v;
  }
  if ((threadIdx.x & 63) == 0 && v) atomicMax(&rec->longest, v);
}

// Exclusive scan of one value per thread over the workgroup, in thread order; *total = the sum.  (two barriers; `tmp` holds kWaves words)
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* tmp, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  __syncthreads();  // (tmp may still be read from an earlier call)
  if (lane == 63) tmp[wave] = inc;
  __syncthreads();
  uint32_t before = 0u, all = 0u;
  for (int w = 0; w < kWaves; ++w) {
    const uint32_t t = tmp[w];
    if (w < wave) before += t;
    all += t;
  }
  *total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(kBlock) void k_ct_block_sums(uint32_t ncell, const uint32_t* __restrict__ count, uint32_t* __restrict__ sums) {
  __shared__ uint32_t wave_sum[kWaves];
  const size_t first = (size_t)blockIdx.x * kPerBlock + (size_t)threadIdx.x * kPerThread;
  uint32_t s = 0u;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j)
    if (first + j < ncell) s += count[first + j];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0u;
    for (int w = 0; w < kWaves; ++w) t += wave_sum[w];
    sums[blockIdx.x] = t;
  }
}
// sums[b] := the sums of the workgroups in front of b.  One workgroup, kBlock entries per pass, the running sum carried along.
__global__ __launch_bounds__(kBlock) void k_ct_scan_sums(int blocks, uint32_t* __restrict__ sums) {
  __shared__ uint32_t tmp[kWaves];
  uint32_t carry = 0u;
  for (int first = 0; first < blocks; first += kBlock) {
    const int b = first + (int)threadIdx.x;
    const uint32_t v = b < blocks ? sums[b] : 0u;
    uint32_t total;
    const uint32_t before = block_exclusive_scan(v, tmp, &total);
    if (b < blocks) sums[b] = carry + before;
    carry += total;
  }
}
// start[c] (behind the front guard cells) := the records in front of cell c; the counters return to zero: the scatter's fill levels
__global__ __launch_bounds__(kBlock) void k_ct_scan_write(uint32_t ncell, uint32_t* __restrict__ count, const uint32_t* __restrict__ sums,
                                                          uint32_t* __restrict__ start_cells) {
  __shared__ uint32_t tmp[kWaves];
  const size_t first = (size_t)blockIdx.x * kPerBlock + (size_t)threadIdx.x * kPerThread;
  uint32_t v[kPerThread], s = 0u;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) v[j] = first + j < ncell ? count[first + j] : 0u, s += v[j];
  uint32_t total;
  uint32_t at = sums[blockIdx.x] + block_exclusive_scan(s, tmp, &total);
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    if (first + j < ncell) start_cells[first + j] = at, count[first + j] = 0u;
    at += v[j];
  }
}
// the cell table's guard cells: `guard` zeros in front, the end of the last cell and `guard` more entries with the total behind
__global__ __launch_bounds__(kBlock) void k_ct_guards(uint32_t guard, uint32_t ncell, uint32_t total, uint32_t* __restrict__ start) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < guard) start[i] = 0u;
  else if (i < 2 * (size_t)guard + 1) start[(size_t)ncell + i] = total;  // entries guard + ncell .. 2 guard + ncell
}

__global__ __launch_bounds__(kBlock) void k_ct_scatter(BuildArgs a, const Node* __restrict__ nodes, const uint32_t* __restrict__ start_cells, uint32_t* __restrict__ fill,
                                                       uint32_t refs, uint32_t* __restrict__ scratch) {
  int i;
  Node n;
  if (!wave_leaf(a, nodes, &i, &n)) return;
  const Range r(n, a);
  for (int k = (int)(threadIdx.x & 63); k < r.total; k += 64) {
    int x, y, z;
    r.cell(k, &x, &y, &z);
    const size_t c = ptct::cell_index(a.frame.res, x, y, z);
    if (c >= (size_t)a.ncell) continue;
    const uint32_t at = start_cells[c] + atomicAdd(&fill[c], 1u);
    if (at < refs) scratch[at] = (uint32_t)i;  // (at < refs by construction; the list holds refs entries)
  }
}

__global__ __launch_bounds__(kBlock) void k_ct_records(BuildArgs a, const Node* __restrict__ nodes, const DeviceGeom* __restrict__ geoms,
                                                       const uint32_t* __restrict__ start_cells, const uint32_t* __restrict__ scratch, uint32_t refs,
                                                       Node* __restrict__ items, Node* __restrict__ items_b) {
  int i;
  Node n;
  if (!wave_leaf(a, nodes, &i, &n)) return;
  const Range r(n, a);
  const int type = geoms[n.geom].type, geom = n.geom;
  Node it = n, itb = n;
  it.skip = itb.skip = i;
  if (a.center_half) ptct::center_half_box(itb.bmin, itb.bmax, false, 0.0);  // the grid's records are leaf boxes
  for (int k = (int)(threadIdx.x & 63); k < r.total; k += 64) {
    int x, y, z;
    r.cell(k, &x, &y, &z);
    const size_t c = ptct::cell_index(a.frame.res, x, y, z);
    if (c >= (size_t)a.ncell) continue;
    const uint32_t s = start_cells[c], e = start_cells[c + 1] < refs ? start_cells[c + 1] : refs;
    uint32_t rank = 0u;
    for (uint32_t j = s; j < e; ++j) rank += scratch[j] < (uint32_t)i ? 1u : 0u;
    if (s + rank >= refs) continue;  // (never: the leaf is one of the cell's e - s entries)
    it.geom = itb.geom = ptct::record_geom_word(x, y, z, r.c0, r.c1, type, geom);
    store32(items + s + rank, it);
    if (a.center_half) store32(items_b + s + rank, itb);
  }
}

// ---- pt_selfcheck_camera_math ------------------------------------------------------------------------------------------------------
// One shared-header function on one operand set; what the kernel and the host loop both run.
PT_HD void math_eval(int kind, const MathOp& o, MathOut& r) {
  for (int k = 0; k < 16; ++k) r.w[k] = 0u;
  if (kind == 0 || kind == 1) {
    const double v = kind == 0 ? ptct::sqrt64(o.d[0]) : ptct::div64(o.d[0], o.d[1]);
    memcpy(&r.w[0], &v, 8);
  } else if (kind == 2) {
    const float f = (float)o.d[0];
    r.w[0] = ptct::bits_of(f), r.w[1] = ptct::bits_of(ptct::next_down(f)), r.w[2] = ptct::bits_of(ptct::next_up(f));
  } else if (kind == 3) {
    for (int inner = 0; inner < 2; ++inner) {
      float lo[3] = {o.f[0], o.f[1], o.f[2]}, hi[3] = {o.f[3], o.f[4], o.f[5]};
      ptct::center_half_box(lo, hi, inner != 0, o.d[0]);
      for (int k = 0; k < 3; ++k) r.w[6 * inner + k] = ptct::bits_of(lo[k]), r.w[6 * inner + 3 + k] = ptct::bits_of(hi[k]);
    }
  } else if (kind == 4) {
    float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
    const bool ok = ptct::sphere_tight_box(o.f, &o.d[0], &o.d[3], &o.f[16], &o.f[19], lo, hi);
    r.w[0] = ok ? 1u : 0u;
    if (ok)
      for (int k = 0; k < 3; ++k) r.w[1 + k] = ptct::bits_of(lo[k]), r.w[4 + k] = ptct::bits_of(hi[k]);
  } else {
    ptct::GridFrame f;
    f.pad = o.d[0];
    for (int k = 0; k < 3; ++k) f.lo[k] = o.d[1 + k], f.ext[k] = o.d[4 + k], f.res[k] = (int)o.f[6 + k];
    int c0[3], c1[3];
    ptct::cell_range(&o.f[0], &o.f[3], f, c0, c1);
    for (int k = 0; k < 3; ++k) r.w[k] = (uint32_t)c0[k], r.w[3 + k] = (uint32_t)c1[k];
  }
}
__global__ __launch_bounds__(kBlock) void k_ct_math(int kind, size_t n, const MathOp* __restrict__ ops, MathOut* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  MathOut r;
  math_eval(kind, ops[i], r);
  out[i] = r;
}

// The operand sets: a fixed list of edge values per kind, then `count` pseudo-random sets from `seed`.
struct Rng {
  uint64_t s;
  uint64_t next() {  // splitmix64
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  double unit() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
  double range(double lo, double hi) { return lo + (hi - lo) * unit(); }
  double bits64() {  // any finite or infinite double, no NaN
    for (;;) {
      const uint64_t u = next();
      double d;
      memcpy(&d, &u, 8);
      if (d == d) return d;
    }
  }
  float scaled(double lo_exp, double hi_exp) { return (float)(range(-1.0, 1.0) * std::pow(2.0, range(lo_exp, hi_exp))); }
};
double from_bits(uint64_t u) {
  double d;
  memcpy(&d, &u, 8);
  return d;
}
const double kInf = __builtin_inf();
const double kEdge64[] = {0.0, -0.0, 4.9406564584124654e-324, 2.2250738585072009e-308 /* largest denormal */, 2.2250738585072014e-308, 1.0, 2.0, 3.0, 4.0, 0.25,
                          1.0000000000000002, 0.99999999999999989, 2.0000000000000004, 1.7976931348623157e308, 8.9884656743115795e307, 1e-320, 1e300, 1e-300,
                          (double)FLT_MAX, (double)FLT_MIN, 1.401298464324817e-45 /* the smallest float denormal */, kInf};
const int kEdges64 = (int)(sizeof(kEdge64) / sizeof(kEdge64[0]));
// doubles around what (float) rounds to +-0, to denormals, to the largest finite float and to infinity
const double kEdgeToFloat[] = {0.0, -0.0, 1.401298464324817e-45, 7.006492321624085e-46 /* half of it: ties to 0 */, 7.0064923216240862e-46, 2.1e-45, 1e-40, 1.1754942e-38,
                               1.17549435e-38, 1e-50, 4.9406564584124654e-324, 1.0, 1.0000000596046448 /* 1 + 2^-24: a tie */, 16777217.0, (double)FLT_MAX,
                               3.4028235677973362e38 /* below the tie to infinity */, 3.4028235677973366e38 /* the tie: to infinity */, 3.5e38, 1e300, kInf};
const int kEdgesToFloat = (int)(sizeof(kEdgeToFloat) / sizeof(kEdgeToFloat[0]));

void identity(float* m, float scale) {
  for (int k = 0; k < 16; ++k) m[k] = 0.f;
  m[0] = m[5] = m[10] = scale, m[15] = 1.f;
}
void sphere_common(MathOp& o, float half_region, float ref_half) {  // origin region and reference box around the origin
  for (int k = 0; k < 3; ++k) o.d[k] = -(double)half_region, o.d[3 + k] = (double)half_region, o.f[16 + k] = -ref_half, o.f[19 + k] = ref_half;
}
void make_operands(int kind, uint64_t count, uint32_t seed, std::vector<MathOp>& ops) {
  ops.clear();
  MathOp z{};
  Rng rng{0x5eed0000ull + seed + ((uint64_t)kind << 40)};
  if (kind == 0) {
    for (int i = 0; i < kEdges64; ++i) ops.push_back(z), ops.back().d[0] = kEdge64[i] < 0.0 ? 0.0 : kEdge64[i];
    ops[1].d[0] = -0.0;
    for (uint64_t i = 0; i < count; ++i) {
      MathOp o = z;
      if (i & 1) {  // a sum of three squares of floats: what the header takes roots of
        const double a = rng.scaled(-20, 20), b = rng.scaled(-20, 20), c = rng.scaled(-20, 20);
        o.d[0] = (a * a + b * b) + c * c;
      } else {
        o.d[0] = std::fabs(rng.bits64());
      }
      ops.push_back(o);
    }
  } else if (kind == 1) {
    for (int i = 0; i < kEdges64; ++i)
      for (int j = 0; j < kEdges64; ++j) {
        ops.push_back(z), ops.back().d[0] = kEdge64[i], ops.back().d[1] = kEdge64[j];
        ops.push_back(z), ops.back().d[0] = -kEdge64[i], ops.back().d[1] = kEdge64[j];
      }
    for (uint64_t i = 0; i < count; ++i) {
      MathOp o = z;
      if (i % 3 == 0) {
        o.d[0] = rng.bits64(), o.d[1] = rng.bits64();
      } else if (i % 3 == 1) {  // a cofactor over a determinant
        const double a = rng.scaled(-10, 10), b = rng.scaled(-10, 10), c = rng.scaled(-10, 10), d = rng.scaled(-10, 10);
        o.d[0] = a * b - c * d, o.d[1] = (double)rng.scaled(-30, 30) * rng.scaled(-10, 10) - (double)rng.scaled(-10, 10);
      } else {  // a cell coordinate over an extent
        o.d[0] = rng.range(-1e3, 1e3), o.d[1] = rng.range(1e-3, 1e3);
      }
      ops.push_back(o);
    }
  } else if (kind == 2) {
    for (int i = 0; i < kEdgesToFloat; ++i) {
      ops.push_back(z), ops.back().d[0] = kEdgeToFloat[i];
      ops.push_back(z), ops.back().d[0] = -kEdgeToFloat[i];
    }
    for (uint64_t i = 0; i < count; ++i) {
      MathOp o = z;
      const uint32_t u = (uint32_t)rng.next();
      const float f = ptct::float_of((u & 0x7f800000u) == 0x7f800000u ? u & 0xff7fffffu : u);  // any float but NaN and infinity
      o.d[0] = (i & 1) ? (double)f : (double)f * (1.0 + rng.range(-1.2e-7, 1.2e-7));            // itself, or a double next to it
      if (i % 16 == 3) o.d[0] = rng.range(-3e-45, 3e-45);                                        // around the smallest denormals
      if (i % 16 == 7) o.d[0] = (double)FLT_MAX * (1.0 + rng.range(-1e-7, 1e-7)) * ((i & 16) ? 1.0 : -1.0);  // around the overflow
      ops.push_back(o);
    }
  } else if (kind == 3) {
    const float e[] = {0.f, -0.f, 1e-45f, -1e-45f, 1e-40f, FLT_MIN, 1.f, -1.f, 16777216.f, FLT_MAX, -FLT_MAX, 3e38f};
    const int ne = (int)(sizeof(e) / sizeof(e[0]));
    for (int i = 0; i < ne; ++i)
      for (int j = 0; j < ne; ++j) {
        if (e[i] > e[j]) continue;
        MathOp o = z;
        for (int k = 0; k < 3; ++k) o.f[k] = e[i], o.f[3 + k] = e[j];
        o.d[0] = (i + j) % 3 == 0 ? 0.0 : (i + j) % 3 == 1 ? 10.5 : 3e6;
        ops.push_back(o);
      }
    ops.push_back(z), ops.back().d[0] = 3.4e38;  // a magnitude whose slack overflows float: the half extent converts to infinity
    for (uint64_t i = 0; i < count; ++i) {
      MathOp o = z;
      const double ex = rng.range(-30, 30);
      for (int k = 0; k < 3; ++k) {
        const float a = rng.scaled(ex - 4, ex), b = (i & 3) == 0 ? a : rng.scaled(ex - 8, ex);
        o.f[k] = a < b ? a : b, o.f[3 + k] = a < b ? b : a;
      }
      o.d[0] = (i & 4) ? std::fabs((double)rng.scaled(ex - 4, ex + 8)) : 0.0;
      ops.push_back(o);
    }
  } else if (kind == 4) {
    const float scales[] = {1.f, 0.f, 1e-30f, 1e30f, 1e-45f, 1e19f, 1e-19f, 3e38f, -2.f};
    for (float s : scales) {
      MathOp o = z;
      identity(o.f, s);
      sphere_common(o, 10.f, 0.5f / (s > 1e-10f && s < 1e10f ? s : 1.f) + 0.25f);
      ops.push_back(o);
    }
    {  // a singular matrix of rank 2 (two equal columns), and one whose cofactors cancel to +-0
      MathOp o = z;
      identity(o.f, 2.f);
      for (int r = 0; r < 3; ++r) o.f[4 + r] = o.f[r];
      sphere_common(o, 10.f, 1.f);
      ops.push_back(o);
      identity(o.f, 1.f);
      o.f[0] = o.f[5] = o.f[10] = 0.f, o.f[1] = 1.f, o.f[4] = -1.f, o.f[10] = -0.f;
      ops.push_back(o);
    }
    {  // a translation so large that centre +- half converts to infinity: the reference box must be kept; and a region of +-FLT_MAX
      MathOp o = z;
      identity(o.f, 1e-20f);
      o.f[12] = 3e38f, o.f[13] = -3e38f, o.f[14] = 1e20f;
      sphere_common(o, 10.f, 1.f);
      ops.push_back(o);
      identity(o.f, 2.f);
      sphere_common(o, FLT_MAX, 1.f);
      ops.push_back(o);
      sphere_common(o, 0.f, 1e-45f);
      ops.push_back(o);
    }
    for (uint64_t i = 0; i < count; ++i) {  // rotation x scale with a translation, the reference box = the unit cube's box, as the scene loader builds it
      MathOp o = z;
      const double ax = rng.range(0, 6.2831853), ay = rng.range(0, 6.2831853), az = rng.range(0, 6.2831853);
      const double sx = std::sin(ax), cx = std::cos(ax), sy = std::sin(ay), cy = std::cos(ay), sz = std::sin(az), cz = std::cos(az);
      const double R[3][3] = {{cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz}, {cy * sz, sx * sy * sz + cx * cz, cx * sy * sz - sx * cz}, {-sy, sx * cy, cx * cy}};
      const double big = (i % 8 == 5) ? rng.range(-20, 20) : rng.range(-3, 3);
      const double sc[3] = {std::pow(2.0, big + rng.range(-2, 2)), std::pow(2.0, big + rng.range(-2, 2)), std::pow(2.0, big + rng.range(-2, 2))};
      const double pos[3] = {rng.range(-20, 20), rng.range(-20, 20), rng.range(-20, 20)};
      // transform = T R S: inverse = S^-1 R^T T^-1, column-major
      for (int r = 0; r < 3; ++r) {
        double t = 0.0;
        for (int c = 0; c < 3; ++c) o.f[c * 4 + r] = (float)(R[c][r] / sc[r]), t -= R[c][r] / sc[r] * pos[c];
        o.f[12 + r] = (float)t;
      }
      o.f[15] = 1.f;
      for (int a = 0; a < 3; ++a) {
        double h = 0.0;
        for (int c = 0; c < 3; ++c) h += std::fabs(R[a][c] * sc[c]) * 0.5;
        const float lo = (float)(pos[a] - h), hi = (float)(pos[a] + h);
        o.f[16 + a] = (i % 8 == 6) ? (float)(pos[a] - 0.1 * h) : lo, o.f[19 + a] = hi;  // (sometimes a reference box that cuts the sphere's)
        o.d[a] = std::fmin(-25.0, (i & 1) ? -25.0 : rng.range(-3000, 0)), o.d[3 + a] = std::fmax(25.0, (i & 2) ? 25.0 : rng.range(0, 3e6));
      }
      ops.push_back(o);
    }
  } else {
    const float e[] = {0.f, -0.f, 1e-45f, 1.f, -1.f, 1e10f, -1e10f, FLT_MAX, -FLT_MAX};
    for (float lo : e)
      for (float hi : e) {
        MathOp o = z;
        for (int k = 0; k < 3; ++k) o.f[k] = lo, o.f[3 + k] = hi, o.f[6 + k] = (float)(1 + 7 * k), o.d[1 + k] = -1.0002, o.d[4 + k] = 2.0004 + k;
        o.d[0] = 1e-4;
        ops.push_back(o);
        o.d[4] = 1e-300, o.d[5] = 4.9406564584124654e-324, o.f[8] = 512.f;  // extents that overflow the quotient
        ops.push_back(o);
      }
    for (uint64_t i = 0; i < count; ++i) {
      MathOp o = z;
      const double ex = rng.range(-10, 20), size = std::pow(2.0, ex);
      o.d[0] = size * rng.range(1e-4, 4e-2);
      for (int k = 0; k < 3; ++k) {
        const double lo = rng.range(-4, 4) * size, ext = size * rng.range(0.05, 1.0) + 4.0 * o.d[0];
        o.d[1 + k] = lo, o.d[4 + k] = ext;
        const int res = 1 + (int)(rng.next() % ((i & 1) ? 512 : 12));
        o.f[6 + k] = (float)res;
        // a box inside the frame, often with a face on a cell boundary (a lattice scene puts them there)
        double a = lo + ext * rng.unit(), b = lo + ext * rng.unit();
        if (i % 4 == 1) a = lo + ext * (double)(rng.next() % (uint64_t)res) / res + o.d[0];
        if (i % 4 == 2) b = lo + ext * (double)(rng.next() % (uint64_t)res) / res - o.d[0];
        o.f[k] = (float)std::fmin(a, b), o.f[3 + k] = (float)std::fmax(a, b);
      }
      ops.push_back(o);
    }
  }
}
bool same_out(int kind, const MathOut& a, const MathOut& b) {
  if (kind <= 1) {  // a NaN result (0 / 0, infinity / infinity) is a NaN on both sides, whatever its sign and payload
    double x, y;
    memcpy(&x, &a.w[0], 8), memcpy(&y, &b.w[0], 8);
    if (x != x && y != y) return true;
  }
  return memcmp(&a, &b, sizeof(MathOut)) == 0;
}

unsigned blocks_of(size_t n, int per) { return (unsigned)((n + per - 1) / per); }
int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : pt_fail("%s: launch failed: %s", who, hipGetErrorString(e));
}
}  // namespace

// pt_internal.h
int pt_camera_tables_nodes_launch(hipStream_t stream, const BuildArgs& a, const Node* base_nodes, const TopEntry* base_top, const DeviceGeom* geoms, Node* nodes,
                                  Node* nodes_b, TopEntry* top, TopEntry* top_b, BuildRecord* rec) {
  if (a.num_nodes < 1 || a.num_top < 0 || a.num_top > ptd::kMaxTop || !base_nodes || !base_top || !geoms || !nodes || !top || !rec ||
      (a.center_half && (!nodes_b || !top_b)))
    return pt_fail("pt_set_camera_ex: bad argument (device tables)");
  if (hipMemsetAsync(rec, 0, sizeof(BuildRecord), stream) != hipSuccess) return pt_fail("pt_set_camera_ex: hipMemsetAsync failed");
  hipLaunchKernelGGL(k_ct_nodes, dim3(blocks_of((size_t)a.num_nodes, kBlock)), dim3(kBlock), 0, stream, a, base_nodes, geoms, nodes, nodes_b, rec);
  if (a.num_top) hipLaunchKernelGGL(k_ct_top, dim3(1), dim3(64), 0, stream, a, base_top, nodes, top, top_b);
  return launched("pt_set_camera_ex");
}

size_t pt_camera_tables_scan_blocks(size_t ncell) { return (ncell + kPerBlock - 1) / kPerBlock; }

int pt_camera_tables_count_launch(hipStream_t stream, const BuildArgs& a, const Node* nodes, uint32_t* count, BuildRecord* rec) {
  if (a.num_nodes < 1 || a.ncell < 1 || (int64_t)a.ncell > ptct::kDeviceMaxCells || !nodes || !count || !rec ||
      (int64_t)a.frame.res[0] * a.frame.res[1] * a.frame.res[2] != (int64_t)a.ncell)
    return pt_fail("pt_set_camera_ex: bad argument (device grid)");
  if (hipMemsetAsync(count, 0, (size_t)a.ncell * sizeof(uint32_t), stream) != hipSuccess) return pt_fail("pt_set_camera_ex: hipMemsetAsync failed");
  hipLaunchKernelGGL(k_ct_refs, dim3(blocks_of((size_t)a.num_nodes, kBlock)), dim3(kBlock), 0, stream, a, nodes, rec);
  hipLaunchKernelGGL(k_ct_count, dim3(blocks_of((size_t)a.num_nodes, kWaves)), dim3(kBlock), 0, stream, a, nodes, rec, count);
  hipLaunchKernelGGL(k_ct_longest, dim3(blocks_of((size_t)a.ncell, kBlock)), dim3(kBlock), 0, stream, a.ncell, count, rec);
  return launched("pt_set_camera_ex");
}

int pt_camera_tables_grid_launch(hipStream_t stream, const BuildArgs& a, const Node* nodes, const DeviceGeom* geoms, uint32_t* count, uint32_t* sums,
                                 uint32_t* scratch, uint32_t refs, uint32_t* start, Node* items, Node* items_b) {
  if (a.num_nodes < 1 || a.ncell < 1 || (int64_t)a.ncell > ptct::kDeviceMaxCells || refs < 1 || (int64_t)refs > ptct::kMaxRefs || !nodes || !geoms || !count ||
      !sums || !scratch || !start || !items || (a.center_half && !items_b))
    return pt_fail("pt_set_camera_ex: bad argument (device grid)");
  const unsigned blocks = (unsigned)pt_camera_tables_scan_blocks(a.ncell);
  uint32_t* start_cells = start + a.guard;
  hipLaunchKernelGGL(k_ct_block_sums, dim3(blocks), dim3(kBlock), 0, stream, a.ncell, count, sums);
  hipLaunchKernelGGL(k_ct_scan_sums, dim3(1), dim3(kBlock), 0, stream, (int)blocks, sums);
  hipLaunchKernelGGL(k_ct_scan_write, dim3(blocks), dim3(kBlock), 0, stream, a.ncell, count, sums, start_cells);
  hipLaunchKernelGGL(k_ct_guards, dim3(blocks_of(2 * (size_t)a.guard + 1, kBlock)), dim3(kBlock), 0, stream, a.guard, a.ncell, refs, start);
  hipLaunchKernelGGL(k_ct_scatter, dim3(blocks_of((size_t)a.num_nodes, kWaves)), dim3(kBlock), 0, stream, a, nodes, start_cells, count, refs, scratch);
  hipLaunchKernelGGL(k_ct_records, dim3(blocks_of((size_t)a.num_nodes, kWaves)), dim3(kBlock), 0, stream, a, nodes, geoms, start_cells, scratch, refs, items, items_b);
  return launched("pt_set_camera_ex");
}

// One kind of pt_selfcheck_camera_math on the current device: *mismatches += operand sets whose results differ in any bit between the
// device and the host (kind 2 also: between the header's next_down / next_up and libm's nextafterf on the host).
int pt_camera_math_check(int kind, uint64_t count, uint32_t seed, uint64_t* mismatches) {
  std::vector<MathOp> ops;
  make_operands(kind, count, seed, ops);
  const size_t n = ops.size();
  MathOp* d_ops = nullptr;
  MathOut* d_out = nullptr;
  std::vector<MathOut> got(n);
  hipError_t e = hipMalloc(&d_ops, n * sizeof(MathOp));
  if (e == hipSuccess) e = hipMalloc(&d_out, n * sizeof(MathOut));
  if (e == hipSuccess) e = hipMemcpy(d_ops, ops.data(), n * sizeof(MathOp), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_ct_math, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, nullptr, kind, n, d_ops, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(got.data(), d_out, n * sizeof(MathOut), hipMemcpyDeviceToHost);
  (void)hipFree(d_ops);
  (void)hipFree(d_out);
  if (e != hipSuccess) return pt_fail("pt_selfcheck_camera_math: %s", hipGetErrorString(e));
  uint64_t bad = 0;
  for (size_t i = 0; i < n; ++i) {
    MathOut want;
    math_eval(kind, ops[i], want);
    bool ok = same_out(kind, want, got[i]);
    if (kind == 2) {
      const float f = (float)ops[i].d[0];
      ok = ok && want.w[1] == ptct::bits_of(std::nextafterf(f, -INFINITY)) && want.w[2] == ptct::bits_of(std::nextafterf(f, INFINITY));
    }
    bad += ok ? 0 : 1;
  }
  *mismatches = bad;
  return 0;
}
