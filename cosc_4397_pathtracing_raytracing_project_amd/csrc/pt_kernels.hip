// pt_kernels.hip — hand-written gfx950 (CDNA4, wave64) kernels of the wavefront
// path tracer.  One persistent grid per stage; SoA path state; BVH + geometry +
// material tables staged in LDS; wave-level ballot/mbcnt compaction.
//
// What each kernel restates (reference paths relative to its repo root):
//   k_generate   generateRayFromCamera   src/pathtrace.cu:270-286
//   k_intersect  computeIntersections    src/pathtrace.cu:288-333, intersectAABB :113-128,
//                box/sphereIntersectionTest src/intersections.h:48-144
//   k_shade      shadeAndExtendRays      src/pathtrace.cu:336-437 (+ helpers :216-242,
//                RNG :203-207, utilhash intersections.h:12-20) fused with the retirement
//                rule of SURVEY.md §8a and the compaction the reference never had
//   k_collect    finalGather             src/pathtrace.cu:439-444 (sums the retirement records, pt_device.h RetireBuf,
//                into the image in iteration order)
//   k_preview    sendImageToPBO          src/pathtrace.cu:250-268
//   k_save_u8    saveImage + savePNG     src/main.cpp:86-107, src/image.cpp:22-39
//   k_features   (no counterpart) first-hit feature buffers: generate + intersect of depth 0 summed per pixel (pt_features.inc)
// and the two kernels the default pipeline actually runs, which fuse the above so that neither the primary ray nor the
// hit record ever goes through HBM, and no path state after depth 0:
//   k_primary    depth 0:  generate + intersect + shade + compaction into one depth-1 list per (queue, iteration)
//   k_paths      ALL depths >= 1 in one launch: persistent lanes with their own depth, a dead lane takes the next
//                depth-1 ray; three search forms (LDS tables / top list + subtree scans / uniform grid walk)
// (k_generate / k_intersect / k_shade remain as the unfused form for stage-parity tests and A/B runs,
// k_intersect_legacy as the per-lane tree walk the wave-cooperative search replaced.)
// Shared: keep_closest / resolve_hit pack and unpack a closest-hit key and record; k_primary's two loop forms go through one front
// end (group_of + trace) and differ in the shading lambda; scan_subtrees is trace_group's and carry_search<true>'s subtree walk.
//
// Arithmetic contract.  This file is compiled once per arithmetic mode (PT_ARITH, see pt_kernels.h KernelApi):
//   0 exact: -ffp-contract=off; every float operation is written in the order GLM 0.9.6 / the reference
//            evaluate it, divisions and square roots are IEEE (hipcc default
//            -fhip-fp32-correctly-rounded-divide-sqrt), and sin/cos/acos come from pt_portable_math.h, so
//            results are bit-identical to oracle/pt_oracle.cpp in PORTABLE mode;
//   1 fma:   the same source with contraction allowed; direction sampling in float only (shade_bounce_float<false>);
//   2 fast:  the `kFast` branches below — hardware rcp / rsq / sqrt / sin / cos, nested-FMA matrix products, FMA slab tests,
//            float-only direction sampling.  Same algorithm, same RNG draws, same decisions; only rounding differs.
// No MFMA: there is no dense contraction here.
#include "pt_kernels.h"

#include <float.h>

#include <type_traits>

#include "pt_lds.h"
#include "pt_sched.h"
#include "pt_portable_math.h"

#ifndef PT_ARITH
#define PT_ARITH 0
#endif
#if PT_ARITH == 0
#define PT_NS arith_exact
#define PT_API_FN api_exact
#elif PT_ARITH == 1
#define PT_NS arith_fma
#define PT_API_FN api_fma
#elif PT_ARITH == 2
#define PT_NS arith_fast
#define PT_API_FN api_fast
#else
#error "PT_ARITH must be 0, 1 or 2"
#endif

namespace ptk {
namespace PT_NS {
namespace {

#define PT_DEV __device__ __forceinline__

constexpr bool kFast = PT_ARITH == 2;
// The fma build samples directions in float only (shade_bounce_float<false>) instead of the exact build's double-reduced form.
constexpr bool kFloatTrig = PT_ARITH == 1;

// Diagnostic builds only (-DPT_WALK_STATS, tools/walk_stats.py): event counts of the large-scene kernels' search loops, added up
// over a launch in a buffer nothing else reads.  The product build compiles none of it.
#ifdef PT_WALK_STATS
__device__ unsigned long long g_walk_stats[16];
#define PT_STAT(i, v)                                                             \
  do {                                                                            \
    const unsigned long long pt_stat_v = (unsigned long long)(v); /* by every lane: v may hold a ballot */ \
    if (lane_id() == 0) atomicAdd(&g_walk_stats[i], pt_stat_v);                   \
  } while (0)
PT_DEV int wave_max_stat(int v) {
  for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
#else
#define PT_STAT(i, v)
#endif

constexpr int kStealMin = 16;  // large-scene (global-table) path: idle lanes needed before a work-stealing step is run (65: never)
// Waves per SIMD the depth-0 kernel is compiled for (__launch_bounds__ second argument).  5: the camera ring's 5.9 KB per wave
// fit five workgroups per CU; in-box, Msamples/s at 4 | 5 | 6: fast 22.5 k | 22.5 k (95 VGPRs either way) | 21.0 k (88 B / lane of
// scratch), fma 17.27 k | 17.45 k, exact 15.29 k | 15.63 k (97 VGPRs at 4; 95 + 20 B / lane of scratch at 5).
constexpr int kPrimaryWaves = 5;

typedef float v4f __attribute__((ext_vector_type(4)));
struct f3 {
  float x, y, z;
};
// ballot() of the HIP headers goes through an integer compare (v_cndmask 0 / 1 + v_cmp per call when the predicate already
// sits in a scalar register pair); the builtin takes the predicate as it is.
PT_DEV unsigned long long ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// mask * 2 + bit in ONE instruction: v_addc_co_u32 takes the predicate as its carry-in (instead of v_mov + v_cndmask + v_or
// per box test).  The bits end up in reverse order of the pushes.
PT_DEV uint32_t push_bit(uint32_t m, bool bit) {
  uint32_t r;
  unsigned long long carry_out;
  asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(r), "=s"(carry_out) : "v"(m), "s"(ballot(bit)));
  return r;
}
// number of set bits of m below this lane
PT_DEV int rank_in(unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0)); }
PT_DEV f3 mk(float x, float y, float z) { return f3{x, y, z}; }

#include "pt_ieee.inc"
// Exact a / n and a % n for 0 <= a < 2^30 and quotients below 2^15 (sample ids / tile pixels,
// pixel index / image width): float estimate + one correction step either way, ~10 VALU instead of
// the ~35 of a 32-bit integer division.  inv_n = 1.0f / n computed once per kernel.
PT_DEV void divmod(int a, int n, float inv_n, int& q, int& r) {
  int k = (int)((float)a * inv_n);
  int rem = a - k * n;
  if (rem < 0) {
    rem += n;
    --k;
  } else if (rem >= n) {
    rem -= n;
    ++k;
  }
  q = k;
  r = rem;
}

// intersectAABB's per-ray constants (see ray_inv in pt_arith.inc)
struct RayInv {
  float ix, iy, iz;
  bool sx, sy, sz;
  float nx, ny, nz;  // fast mode: -origin * reciprocal, so that (b - o) / d is one FMA per plane
};

}  // namespace

// The arithmetic, twice (see pt_arith.inc).  Primary rays are identical in every iteration of a pixel, so a rounding
// difference that flips one of their decisions — the image diagonals of the square cornell frame look exactly along
// the box's corner edges, where two walls tie to the last bit of t — would repeat in every sample of that pixel instead
// of averaging out; measured: 90 % of all fma-vs-reference sample flips at 256 x 256 are such depth-0 ties.  Depth 0
// therefore runs the reference's exact primitive tests (namespace ex) in every arithmetic mode; the stochastic
// bounces use the mode's arithmetic (namespace md).
#pragma clang fp contract(off)
namespace ex {
namespace {
constexpr bool kFastArith = false, kFusedRef = false;
#include "pt_arith.inc"
}  // namespace
}  // namespace ex
#if PT_ARITH != 0
#pragma clang fp contract(fast)
#endif
namespace md {
namespace {
constexpr bool kFastArith = kFast, kFusedRef = PT_ARITH == 1;
#include "pt_arith.inc"
}  // namespace
}  // namespace md
namespace {
using namespace md;
// Arithmetic flavour of a call site: Ar<true> = the reference's exact arithmetic (namespace ex), Ar<false> = the
// build's mode.  kD0 selects the flavour of everything geometric at depth 0; in the exact build both are the same
// arithmetic, so it stays on md and nothing is instantiated twice.
constexpr bool kD0 = PT_ARITH != 0;
template <bool EX>
struct Ar {
  static PT_DEV RayInv ray_inv(f3 d, f3 o) { if constexpr (EX) return ex::ray_inv(d, o); else return md::ray_inv(d, o); }
  static PT_DEV bool slab(f3 o, const RayInv& ri, float a, float b, float c, float d, float e, float f) {
    if constexpr (EX) return ex::slab(o, ri, a, b, c, d, e, f); else return md::slab(o, ri, a, b, c, d, e, f);
  }
  static PT_DEV bool slab_rel(const RayInv& ri, float a, float b, float c, float d, float e, float f) {
    if constexpr (EX) return ex::slab_rel(ri, a, b, c, d, e, f); else return md::slab_rel(ri, a, b, c, d, e, f);
  }
  static PT_DEV bool slab_t(f3 o, const RayInv& ri, float a, float b, float c, float d, float e, float f, float& tn) {
    if constexpr (EX) return ex::slab_t(o, ri, a, b, c, d, e, f, tn); else return md::slab_t(o, ri, a, b, c, d, e, f, tn);
  }
  template <int TYPE, bool QO, bool DEFER = false>
  static PT_DEV float geom_test(const ptd::Geom* __restrict__ G, f3 ro, f3 rd, f3& point, f3& normal, f3 qo_pre, int rt_type = -1) {
    if constexpr (EX) return ex::geom_test<TYPE, QO, DEFER>(G, ro, rd, point, normal, qo_pre, rt_type);
    else return md::geom_test<TYPE, QO, DEFER>(G, ro, rd, point, normal, qo_pre, rt_type);
  }
  static PT_DEV f3 finish_normal(const ptd::Geom* __restrict__ G, f3 stored) {
    if constexpr (EX) return ex::finish_normal(G, stored); else return md::finish_normal(G, stored);
  }
  static PT_DEV f3 camera_dir(const ptd::Camera& cam, float inv_w, int p, bool aa, float jx, float jy) {
    if constexpr (EX) return ex::camera_dir(cam, inv_w, p, aa, jx, jy); else return md::camera_dir(cam, inv_w, p, aa, jx, jy);
  }
  static PT_DEV f3 xf_point(const float* m, f3 v) { if constexpr (EX) return ex::mulMV<1>(m, v); else return md::mulMV<1>(m, v); }
};

PT_DEV int lane_id() { return (int)(threadIdx.x & 63); }
// value of v in lane src_lane
PT_DEV float bperm(int src_lane, float v) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane << 2, __float_as_int(v)));
}

// ───────────────────────────── RNG ──────────────────────────────────────────
PT_DEV uint32_t utilhash(uint32_t a) {  // intersections.h:12-20
  a = (a + 0x7ed55d16u) + (a << 12);
  a = (a ^ 0xc761c23cu) ^ (a >> 19);
  a = (a + 0x165667b1u) + (a << 5);
  a = (a + 0xd3a2646cu) ^ (a << 9);
  a = (a + 0xfd7046c5u) + (a << 3);
  a = (a ^ 0xb55a4f09u) ^ (a >> 16);
  return a;
}
// thrust::minstd_rand (a = 48271, m = 2^31 - 1) with Mersenne folding instead of %.
struct MinStd {
  uint32_t x;
  PT_DEV explicit MinStd(uint32_t s) {
    uint32_t r = (s & 0x7fffffffu) + (s >> 31);  // s mod (2^31-1)
    if (r >= 0x7fffffffu) r -= 0x7fffffffu;
    x = r == 0u ? 1u : r;
  }
  PT_DEV uint32_t next() {
    uint64_t p = (uint64_t)x * 48271u;  // < 2^47
    uint32_t r = (uint32_t)(p & 0x7fffffffu) + (uint32_t)(p >> 31);
    if (r >= 0x7fffffffu) r -= 0x7fffffffu;
    x = r;
    return r;
  }
  // uniform_real_distribution<float>(0,1): float(x - 1) / 2^31 (exact scaling)
  PT_DEV float u01() { return (float)(next() - 1u) * 4.656612873077392578125e-10f; }
};
// makeSeededRandomEngine (pathtrace.cu:203-207): seed = utilhash((1 << 31) | (depth << 22) | iter) ^ utilhash(index).
// The first factor depends only on (iteration, depth): the kernels compute it once per iteration of the batch into
// a small LDS table (pt_lds.h iter_hash_entries) instead of once per ray (same values, ~18 VALU less per ray).
PT_DEV uint32_t iter_hash(int iter, int depth) { return utilhash((1u << 31) | ((uint32_t)depth << 22) | (uint32_t)iter); }
PT_DEV void iter_hash_fill(uint32_t* tab, const SceneTables& sc, const BatchInfo& b, int depth) {  // before the kernel's __syncthreads()
  if (iter_hash_entries(sc) > 0)
    for (int i = threadIdx.x; i < b.K; i += blockDim.x) tab[i] = iter_hash(b.iter_first + i, depth);
}
PT_DEV uint32_t iter_hash_of(const uint32_t* tab, const SceneTables& sc, const BatchInfo& b, int depth, int k) {
  return iter_hash_entries(sc) > 0 ? tab[k] : iter_hash(b.iter_first + k, depth);
}

// Anti-aliasing jitter of sample (iteration, global pixel): two draws of an engine seeded in a hash domain of its own
// ("depth" field 0x100: bit 30, which no path depth < 64 produces), so the streams of the reference semantics are untouched.
PT_DEV void aa_jitter(int iter, int pixel, float& jx, float& jy) {
  MinStd rng(utilhash((1u << 31) | (1u << 30) | (uint32_t)iter) ^ utilhash((uint32_t)pixel));
  jx = rng.u01() - 0.5f;
  jy = rng.u01() - 0.5f;
}

// ───────────────────────────── LDS staging ─────────────────────────────────
// Copies `bytes` (multiple of 16) from global to LDS with 16-B accesses.
PT_DEV void stage16(void* lds, const void* g, int bytes) {
  const float4* src = reinterpret_cast<const float4*>(g);
  float4* dst = reinterpret_cast<float4*>(lds);
  for (int i = threadIdx.x; i < bytes / 16; i += blockDim.x) dst[i] = src[i];
}

// Tile pixel → global pixel index (what keys the RNG and the camera ray), see BatchInfo::stripe and BatchInfo::list (p < b.N).
struct PixelMap {  // the fields of BatchInfo that global_pixel reads
  int pixel_begin, stripe, gap;
  float inv_stripe;
  const int32_t* list;
};
PT_DEV PixelMap pixel_map(const BatchInfo& b) { return PixelMap{b.pixel_begin, b.stripe, b.gap, b.inv_stripe, b.list}; }
PT_DEV int global_pixel(const PixelMap& b, int p) {
  if (b.stripe == 0) return b.pixel_begin + p;
  if (b.list) return b.pixel_begin + b.list[p];  // (the host gives a list batch stripe != 0, so the contiguous form pays nothing for this test)
  int i, r;
  divmod(p, b.stripe, b.inv_stripe, i, r);
  return b.pixel_begin + p + i * b.gap;
}
PT_DEV int global_pixel(const BatchInfo& b, int p) { return global_pixel(pixel_map(b), p); }

// ───────────────────────────── path records (ptd::PathBuf) ─────────────────
// What rides along with a path besides its ray and colour: the sample id.  (phash / k: the per-pixel half of the RNG seed and the
// iteration inside the batch, kept in registers by the kernels that have them; they are not part of the record in memory — a
// round-3 build that carried them, 48 B per path, saved 56 VALU per 64-ray group and was 10-20 % slower.)
struct PathTag {
  int slot;
  uint32_t phash;  // utilhash(global pixel index)
  int k;           // iteration inside the batch: iteration = BatchInfo::iter_first + k
};
struct PathRec {
  f3 o, d, c;
  PathTag tag;
};
struct alignas(8) Word2 {
  float x, y;
};
// plane 2: colour.z, slot
PT_DEV void plane2_load(const ptd::PathBuf& b, int64_t at, float& cz, PathTag& tag) {
  const Word2 w2 = reinterpret_cast<const Word2*>(b.r + 2 * b.stride)[at];
  cz = w2.x;
  tag.slot = __float_as_int(w2.y), tag.phash = 0u, tag.k = 0;
}
PT_DEV void plane2_store(const ptd::PathBuf& b, int64_t at, float cz, const PathTag& tag) {
  reinterpret_cast<Word2*>(b.r + 2 * b.stride)[at] = Word2{cz, __int_as_float(tag.slot)};
}
PT_DEV void path_load_ray(const ptd::PathBuf& b, int64_t at, f3& o, f3& d) {  // planes 0, 1
  const ptd::Word4 w0 = b.r[at], w1 = b.r[b.stride + at];
  o = mk(w0.x, w0.y, w0.z);
  d = mk(w0.w, w1.x, w1.y);
}
PT_DEV void path_load_tail(const ptd::PathBuf& b, int64_t at, f3& d, f3& c, PathTag& tag) {  // planes 1, 2 + direction.x
  const ptd::Word4 w1 = b.r[b.stride + at];
  float cz;
  plane2_load(b, at, cz, tag);
  d = mk(reinterpret_cast<const float*>(b.r + at)[3], w1.x, w1.y);
  c = mk(w1.z, w1.w, cz);
}
PT_DEV PathRec path_load(const ptd::PathBuf& b, int64_t at) {
  const ptd::Word4 w0 = b.r[at], w1 = b.r[b.stride + at];
  PathRec v;
  float cz;
  plane2_load(b, at, cz, v.tag);
  v.o = mk(w0.x, w0.y, w0.z);
  v.d = mk(w0.w, w1.x, w1.y);
  v.c = mk(w1.z, w1.w, cz);
  return v;
}
PT_DEV void path_store(const ptd::PathBuf& b, int64_t at, f3 o, f3 d, f3 c, const PathTag& tag) {
  b.r[at] = ptd::Word4{o.x, o.y, o.z, d.x};
  b.r[b.stride + at] = ptd::Word4{d.y, d.z, c.x, c.y};
  plane2_store(b, at, c.z, tag);
}
// Iteration (inside the batch) and tile pixel of a path from its sample id k << slot_shift | pl (BatchInfo::slot_shift: a
// shift and a mask instead of the division by N that the id k * N + pl of rounds 1-2 needed at every depth).
PT_DEV int make_slot(const BatchInfo& b, int k, int pl) { return (k << b.slot_shift) | pl; }
PT_DEV void sample_of(const PathTag& tag, const BatchInfo& b, int& k, int& pl) {
  k = (int)((uint32_t)tag.slot >> b.slot_shift);
  pl = tag.slot & ((1 << b.slot_shift) - 1);
}
// makeSeededRandomEngine's seed (pathtrace.cu:205) of a path at `depth`: utilhash((1 << 31) | depth << 22 | iteration) ^
// utilhash(global pixel index).  The first factor comes from the per-block table (iter_hash_of).
PT_DEV uint32_t path_seed(int k, int pl, const uint32_t* ihash, const SceneTables& sc, const BatchInfo& b, int depth) {
  return iter_hash_of(ihash, sc, b, depth, k) ^ utilhash((uint32_t)global_pixel(b, pl));
}

// ───────────────────────────── retirement records (ptd::RetireBuf) ─────────
// One queue's regions and counters (pt_device.h RetireBuf).
struct Retire {
  ptd::Word4* rec;          // region (q, 0); region (q, k) starts k * seg_cap records further
  unsigned long long* sub;  // [kmax][wq0]: retirees << 32 | survivors of depth 0 per sub-region / sub-list (q, k, rho)
  unsigned long long* cnt;  // [kmax]: flat form — records appended at the front of region (q, k) << 32
  int seg_cap, wq0;
};
PT_DEV Retire retire_of(const ptd::RetireBuf& rb, int q) {
  Retire rt;
  rt.rec = rb.rec + (int64_t)q * rb.kmax * rb.seg_cap;
  rt.sub = rb.sub + (int64_t)q * rb.kmax * rb.wq0;
  rt.cnt = rb.cnt + (int64_t)q * rb.kmax;
  rt.seg_cap = rb.seg_cap, rt.wq0 = rb.wq0;
  return rt;
}
PT_DEV void retire_store(const Retire& rt, bool dead, int k, int pos, int pl, f3 c) {
  if (dead) rt.rec[(int64_t)k * rt.seg_cap + pos] = ptd::Word4{c.x, c.y, c.z, __int_as_float(pl)};
}
// The unfused stage kernels: every record appended at the front of its region, one returning atomic per record on the
// region's counter (test / A-B form; the fused kernels take one atomic per 64 samples or none at all).
PT_DEV void retire_append(const Retire& rt, bool dead, int k, int pl, f3 c) {
  if (dead) retire_store(rt, true, k, (int)(atomicAdd(&rt.cnt[k], 1ull << 32) >> 32), pl, c);
}

// ───────────────────────────── generate ────────────────────────────────────
__global__ __launch_bounds__(kBlock) void k_generate(ptd::Camera cam, BatchInfo b, ptd::Queues qs, ptd::PathBuf out,
                                                     int32_t* __restrict__ cnt0) {
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int lane = lane_id();
  const auto [q, r, wq] = wave_slot(wave, qs.Q, qs.W);
  const float inv_w = 1.0f / (float)cam.res_x;
  const QueueShare sh = queue_share(b, qs, q);
  if (r == 0 && lane == 0) cnt0[cnt_index(qs, 0, q)] = b.K * sh.my_pixels;
  const int entries = b.K * sh.my_nq;  // iteration-major: entry j = k * my_nq + jj is chunk q + jj * Q of iteration k
  for (int j = r; j < entries; j += wq) {
    int k, jj;
    divmod(j, sh.my_nq, sh.inv_my_nq, k, jj);
    const int pl = chunk_pixel(q, jj, qs.Q) + lane;  // tile pixel
    if (pl < b.N) {
      const int p = global_pixel(b, pl);  // global pixel index
      float jx = 0.f, jy = 0.f;
      if (b.aa_jitter) aa_jitter(b.iter_first + k, p, jx, jy);
      const f3 d = Ar<kD0>::camera_dir(cam, inv_w, p, b.aa_jitter != 0, jx, jy);
      const int64_t at = (int64_t)q * qs.cap + (int64_t)k * sh.my_pixels + jj * 64 + lane;  // dense: a partial chunk is the queue's last
      path_store(out, at, mk(cam.pos[0], cam.pos[1], cam.pos[2]), d, mk(1.0f, 1.0f, 1.0f), PathTag{make_slot(b, k, pl), utilhash((uint32_t)p), k});
    }
  }
}

// ───────────────────────────── intersect ───────────────────────────────────
struct HitRec {
  float t;
  f3 n;
  f3 p;
  int geom;
};

// Near-first order of a ray's entered subtrees.  When the top list is a complete level of a balanced tree its
// entries are laid out by path code (bit 4 = child taken at the root, ... bit 0 = at level 4; pt_tables.cpp build_top),
// so visiting the nearer child first at every level is visiting the entries in increasing (index XOR m) order,
// where bit l of m says that the nearer child at that level is child 1 for this ray's direction signs
// (SceneTables::top_xor, one mask per sign octant).  permute_xor returns the pending mask re-indexed by
// j = e ^ m, so that ctz yields the entries nearest first; the cull then prunes the farther ones earlier.
// Any m is valid (the order never changes results); m = 0 keeps the list order.
PT_DEV uint32_t permute_xor(uint32_t x, uint32_t m) {
  if (m & 1u) x = ((x & 0x55555555u) << 1) | ((x >> 1) & 0x55555555u);
  if (m & 2u) x = ((x & 0x33333333u) << 2) | ((x >> 2) & 0x33333333u);
  if (m & 4u) x = ((x & 0x0f0f0f0fu) << 4) | ((x >> 4) & 0x0f0f0f0fu);
  if (m & 8u) x = ((x & 0x00ff00ffu) << 8) | ((x >> 8) & 0x00ff00ffu);
  if (m & 16u) x = (x << 16) | (x >> 16);
  return x;
}
PT_DEV uint32_t octant_mask(const RayInv& ri, unsigned long long top_xor) {
  const int oct = (int)ri.sx | ((int)ri.sy << 1) | ((int)ri.sz << 2);
  return (uint32_t)(top_xor >> (oct * 8)) & 31u;
}

// One step of a lane's stackless subtree scan.  On return `cur` is advanced, `cand` says whether the node is a
// leaf whose box the ray passes (and that is not culled), `leaf` is its index in `nodes`, `geom` its geom index.
// bt: the ray's best hit distance so far + SceneTables::cull_margin (closer-hit cull).
template <bool EX = false, typename NP = const v4f*>
PT_DEV void scan_step(NP nodes4, f3 o, const RayInv& ri, bool act, int& cur, float bt,
                      bool& cand, int& leaf, int& geom) {
  const int at_n = act ? cur : 0;
  const v4f NA = nodes4[2 * at_n];      // bmin.xyz, bmax.x
  const v4f NB = nodes4[2 * at_n + 1];  // bmax.yz, skip, geom
  float tn;
  const bool in = act && Ar<EX>::slab_t(o, ri, NA.x, NA.y, NA.z, NA.w, NB.x, NB.y, tn) && !(tn > bt);
  geom = __float_as_int(NB.w);
  cand = in && geom >= 0;
  leaf = at_n;
  if (act) cur = in ? cur + 1 : __float_as_int(NB.z);
}

// State of a lane's subtree scan: the subtree range being scanned and the ray it is scanned for (the lane's own
// ray, or a donor's after a steal — see steal_step).
struct Walker {
  int cur, end;  // next node / one past the subtree's last node (cur >= end: idle)
  int own;       // lane that owns the ray (candidates are filed under it)
  f3 o;          // ray origin
  RayInv ri;     // reciprocal direction
};
// Work stealing inside the wave.  The scan loop runs max-over-lanes steps, and lanes' totals range from 0 to several
// hundred node visits (rays enter 0-10 subtrees, a subtree costs 5-150 visits), so lanes whose own pending list
// is empty take one pending (ray, subtree) pair each from lanes that still have some: donors publish their lane id
// in `slot` (64 ints of LDS) by rank, the k-th idle lane reads the k-th donor's id, fetches its pending mask, XOR
// mask, ray origin and reciprocal direction with ds_bpermute, and the donor drops the pair it gave away.
// Called at wave-uniform control flow.  A lane only steals once its own list is empty, hence a donor's Walker
// always holds the donor's own ray.  pend: pending subtrees in permute_xor order.
PT_DEV void steal_step(Walker& w, uint32_t& pend, uint32_t xm, bool idle, unsigned long long I, int* slot,
                       const float4* top, int lane) {
  const unsigned long long Dn = ballot(pend != 0);
  if (!Dn) return;
  const int nd = __popcll(Dn), ni = __popcll(I);
  const int drank = rank_in(Dn);
  const int irank = rank_in(I);
  if (pend != 0) slot[drank] = lane;  // the k-th donor's lane id
  const bool take = idle && irank < nd;
  const int donor = slot[take ? irank : 0];
  const uint32_t dpend = (uint32_t)__builtin_amdgcn_ds_bpermute(donor << 2, (int)pend);
  const int dxm = __builtin_amdgcn_ds_bpermute(donor << 2, (int)xm);
  const f3 so = mk(bperm(donor, w.o.x), bperm(donor, w.o.y), bperm(donor, w.o.z));
  const f3 si = mk(bperm(donor, w.ri.ix), bperm(donor, w.ri.iy), bperm(donor, w.ri.iz));
  if (pend != 0 && drank < ni) pend &= pend - 1;  // given away
  if (take) {
    const int e = __builtin_ctz(dpend) ^ dxm;
    const float4 TB = top[2 * e + 1];
    w.cur = __float_as_int(TB.z) + 1;  // the subtree root's box is the top entry's box: already passed
    w.end = __float_as_int(TB.w);
    w.own = donor;
    w.o = so;
    w.ri.ix = si.x, w.ri.iy = si.y, w.ri.iz = si.z;
    w.ri.sx = si.x < 0.0f, w.ri.sy = si.y < 0.0f, w.ri.sz = si.z < 0.0f;
    w.ri.nx = -so.x * si.x, w.ri.ny = -so.y * si.y, w.ri.nz = -so.z * si.z;
  }
}
// The subtree scans of one group: every lane walks the subtrees its ray entered (`pend`: their top entries) back to back,
// independently of the others, nearest first; lanes without work steal pending (ray, subtree) pairs (steal_step, donor table
// `slot`).  scan(walker, act, bt, cand, leaf, geom) is one scan_step on the caller's node table; file(cand, leaf, owner, geom)
// files a candidate under the lane that owns its ray — wave-uniform control flow, so the primitive tests downstream fetch the
// ray from the owner as for a top-list leaf.  best: the group's closest-hit keys (the closer-hit cull reads the owner's).
// (PT_WALK_STATS builds: counters 1-3 also count trace_group's scans; tools/walk_stats.py runs the fused kernels, i.e. carry_search's.)
template <typename Scan, typename File>
PT_DEV void scan_subtrees(uint32_t pend, const float4* top, f3 o, const RayInv& ri, int lane, unsigned long long top_xor, float cull,
                          const unsigned long long* best, int* slot, Scan scan, File file) {
  if (!ballot(pend != 0)) return;
  Walker wk{0, 0, lane, o, ri};
  const uint32_t xm = octant_mask(ri, top_xor);
  pend = permute_xor(pend, xm);
  while (true) {
    if (wk.cur >= wk.end && pend) {  // own subtrees first, nearest first
      const int e = __builtin_ctz(pend) ^ (int)xm;
      pend &= pend - 1;
      const float4 TB = top[2 * e + 1];
      wk.cur = __float_as_int(TB.z) + 1;  // the subtree root's box is the top entry's box: already passed
      wk.end = __float_as_int(TB.w);
    }
    const bool idle = wk.cur >= wk.end;
    const unsigned long long I = ballot(idle);
    if (I == ~0ull) break;
    if (__popcll(I) >= kStealMin) {
      PT_STAT(3, 1);
      steal_step(wk, pend, xm, idle, I, slot, top, lane);
    }
    const bool act = wk.cur < wk.end;
    PT_STAT(1, 1);
    PT_STAT(2, __popcll(ballot(act)));
    // closer-hit cull: a box entered beyond the ray's best hit so far (+ margin, see SceneTables::cull_margin)
    // cannot hold the closest hit
    const float bt = __uint_as_float(reinterpret_cast<const uint32_t*>(best)[2 * wk.own + 1]) + cull;
    bool cand;
    int at_n, aux;
    scan(wk, act, bt, cand, at_n, aux);
    file(cand, at_n, wk.own, aux);
  }
}
// Legacy traversal (kept for A/B measurements, PtOptions flag): one lane walks the threaded
// tree and runs each primitive test as soon as the wave reaches it.
template <bool EX>
PT_DEV HitRec trace(const ptd::Node* __restrict__ nodes, int num_nodes, const ptd::Geom* __restrict__ geoms, f3 o, f3 d) {
  HitRec h;
  h.t = FLT_MAX;
  h.geom = -1;
  h.n = mk(0.f, 0.f, 0.f);
  h.p = mk(0.f, 0.f, 0.f);
  const RayInv ri = Ar<EX>::ray_inv(d, o);
  int i = 0;
  while (true) {
    int g = -1;
    while (i < num_nodes) {
      const float4 A = reinterpret_cast<const float4*>(nodes)[2 * i];      // bmin.xyz, bmax.x
      const float4 B = reinterpret_cast<const float4*>(nodes)[2 * i + 1];  // bmax.yz, skip, geom
      if (!Ar<EX>::slab(o, ri, A.x, A.y, A.z, A.w, B.x, B.y)) {
        i = __float_as_int(B.z);
        continue;
      }
      i = i + 1;
      const int leaf = __float_as_int(B.w);
      if (leaf >= 0) {
        g = leaf;
        break;
      }
    }
    if (g < 0) break;
    f3 pt, nrm;
    const float t = Ar<EX>::template geom_test<-1, false>(geoms + g, o, d, pt, nrm, mk(0.f, 0.f, 0.f));
    if (t > 0.f && t < h.t) {  // strict <: first found wins ties (pathtrace.cu:314)
      h.t = t;
      h.geom = g;
      h.p = pt;
      h.n = nrm;
    }
  }
  return h;
}

template <bool TABLES_IN_LDS, bool EX>
__global__ __launch_bounds__(kBlock) void k_intersect_legacy(SceneTables sc, ptd::Queues qs,
                                                             const int32_t* __restrict__ cnt_in, ptd::PathBuf paths,
                                                             ptd::HitBuf hits) {
  extern __shared__ float4 lds_raw[];
  const ptd::Node* nodes = EX ? sc.nodes : sc.nodes_b;  // EX: primary rays, the reference's arithmetic on the reference's boxes; else the build's bounce tables
  const ptd::Geom* geoms = sc.geoms;
  if (TABLES_IN_LDS) {
    char* lds = reinterpret_cast<char*>(lds_raw);
    const LegacyLds L = legacy_lds<TABLES_IN_LDS>(sc);
    stage16(lds + L.nodes, nodes, node_bytes(sc));
    stage16(lds + L.geoms, sc.geoms, geom_bytes(sc));
    __syncthreads();
    nodes = reinterpret_cast<const ptd::Node*>(lds + L.nodes);
    geoms = reinterpret_cast<const ptd::Geom*>(lds + L.geoms);
  }
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int lane = lane_id();
  const auto [q, r, wq] = wave_slot(wave, qs.Q, qs.W);
  const int n_q = cnt_in[cnt_index(qs, 0, q)];
  const int64_t HS = hits.stride;
  for (int j = r; j * 64 < n_q; j += wq) {
    const int i = j * 64 + lane;
    if (i < n_q) {
      const int64_t at = (int64_t)q * qs.cap + i;
      f3 o, d;
      path_load_ray(paths, at, o, d);
      const HitRec h = trace<EX>(nodes, sc.num_nodes, geoms, o, d);
      const bool hit = h.geom >= 0;
      // record layout of the reference after its per-depth memset (pathtrace.cu:562):
      // miss → t = -1 and zeros elsewhere.
      hits.t[at] = hit ? h.t : -1.0f;
      hits.n[at] = h.n.x, hits.n[HS + at] = h.n.y, hits.n[2 * HS + at] = h.n.z;
      hits.mat[at] = hit ? geoms[h.geom].material : 0;
      hits.p[at] = h.p.x, hits.p[HS + at] = h.p.y, hits.p[2 * HS + at] = h.p.z;
    }
  }
}

// ── computeIntersections, wave-cooperative form ──────────────────────────────────────────
// Per group of 64 rays a wave runs
//   phase 1  candidate search: every lane tests its ray against the flattened BVH top (box data
//            wave-uniform → scalar loads) and walks entered subtrees with the stackless scan;
//            each (ray, leaf) whose AABB test passes is appended to a per-wave LDS list with a
//            ballot + mbcnt prefix — cubes from the front, spheres from the back;
//   phase 2  primitive tests over the list in dense 64-entry chunks, so all lanes run the same
//            (type-specialised) code on useful work; the ray is fetched from its owner lane with
//            ds_bpermute; the closest hit per ray is kept with an LDS 64-bit atomic min on
//            (t bits << 32 | leaf index).  The reference takes a hit iff t > 0 && t < t_min in its
//            DFS visiting order (pathtrace.cu:314), i.e. the smallest t and, among equal t, the
//            leaf visited first; leaves are numbered in that order, so the key's minimum is
//            exactly the reference's choice no matter in which order candidates are evaluated.
// The reference has no t_min culling, so the candidate set does not depend on hit results and
// the two phases are independent.
struct WaveLds {
  unsigned long long* best;  // [64]
  float* rec;                // [7][64]: normal xyz, point xyz; row 6: donor table of the work-stealing step
  uint32_t* list;            // [kCandCap]: (leaf index << 6) | owner lane
};
PT_DEV WaveLds wave_lds_init(char* base) {  // on a WaveMap::bytes block
  WaveLds w;
  w.best = reinterpret_cast<unsigned long long*>(base + WaveMap::best);
  w.rec = reinterpret_cast<float*>(base + WaveMap::rec);
  w.list = reinterpret_cast<uint32_t*>(base + WaveMap::list);
  return w;
}
constexpr unsigned long long kNoHit = ((unsigned long long)0x7f7fffffu << 32) | 0xffffffffull;  // t_min = FLT_MAX
// Keep the closest hit of a ray: `best_slot` its key, rec + col its column of a [6][64] record block (normal xyz, point xyz).
// A candidate counts iff t > 0 && t < FLT_MAX (pathtrace.cu:314 with t_min starting at FLT_MAX).
// (run_chunk passes block + owner lane, carry_chunk the column and col = 0, each the address arithmetic it had: with the column
// run_chunk's callers k_features<true, false> and k_primary<kTopScan> lose a wave of occupancy, with block + lane k_paths<kGrid> spills.)
PT_DEV void keep_closest(unsigned long long* best_slot, float* rec, int col, float t, uint32_t leaf, f3 nrm, f3 pt, bool valid) {
  const uint32_t tb = __float_as_uint(t);
  if (valid && t > 0.f && tb < 0x7f7fffffu) {
    const unsigned long long key = ((unsigned long long)tb << 32) | leaf;
    atomicMin(best_slot, key);
    if (*best_slot == key) {  // this candidate is the ray's best so far: publish its record
      rec[0 * 64 + col] = nrm.x, rec[1 * 64 + col] = nrm.y, rec[2 * 64 + col] = nrm.z;
      rec[3 * 64 + col] = pt.x, rec[4 * 64 + col] = pt.y, rec[5 * 64 + col] = pt.z;
    }
  }
}
// A ray's closest hit as the shading takes it: t = -1, material 0 and zeros on a miss (the reference's hit record after its
// per-depth memset, pathtrace.cu:562).
struct Hit {
  bool hit;
  float t;
  int geom, mat;
  f3 n, p;
};
// The usual way from a hit's leaf to its geom and material: through the threaded node.  FINISH: the chunks left the world-space
// normal to the winner (carry_chunk, LEAN: the grid walk), in the arithmetic EX.
template <bool FINISH = false, bool EX = false>
struct LeafGeom {
  const ptd::Node* nodes;
  const ptd::Geom* geoms;
  PT_DEV void operator()(uint32_t leaf, Hit& h) const {
    h.geom = nodes[leaf].geom;
    const ptd::Geom* G = geoms + h.geom;
    h.mat = G->material;
    if constexpr (FINISH) h.n = Ar<EX>::finish_normal(G, h.n);
  }
};
// Unpacks a closest-hit key (keep_closest) and its record for the lanes that `want` it; look(leaf, hit) fills in geom and
// material (LeafGeom, or a table of the caller's).
template <typename Look>
PT_DEV Hit resolve_hit(unsigned long long best, const float* rec, bool want, Look look) {
  Hit h{false, -1.0f, -1, 0, mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 0.f)};
  if (want && (uint32_t)(best >> 32) != 0x7f7fffffu) {
    h.hit = true;
    h.t = __uint_as_float((uint32_t)(best >> 32));
    h.n = mk(rec[0 * 64], rec[1 * 64], rec[2 * 64]);
    h.p = mk(rec[3 * 64], rec[4 * 64], rec[5 * 64]);
    look((uint32_t)best, h);
  }
  return h;
}

// Runs the pending candidates; called at wave-uniform control flow with all 64 lanes active.
// One chunk of <= 64 candidates: `nc` cubes starting at list[cfirst] followed by `nsph` spheres starting at
// list[sfirst].  TYPE 1 / 0: the chunk holds only cubes / only spheres (specialised code); TYPE -1: both —
// the object-space transform of the ray and the world-space reconstruction are executed once for all
// lanes and only the slab / quadratic middle parts diverge (geom_test<-1>).
// CAM (primary kernel): every ray starts at the camera, so the origin needs no fetch.
template <int TYPE, bool CAM, bool EX>
PT_DEV void run_chunk(const WaveLds& w, int cfirst, int nc, int sfirst, int nsph, int lane, f3 o, f3 d,
                      const ptd::Node* __restrict__ nodes, const ptd::Geom* __restrict__ geoms) {
  const bool valid = lane < nc + nsph;
  const uint32_t entry = valid ? w.list[lane < nc ? cfirst + lane : sfirst + (lane - nc)] : (uint32_t)lane;
  const int src = (int)(entry & 63u);
  const uint32_t leaf = entry >> 6;
  const f3 ro = CAM ? o : mk(bperm(src, o.x), bperm(src, o.y), bperm(src, o.z));
  const f3 rd = mk(bperm(src, d.x), bperm(src, d.y), bperm(src, d.z));
  const int gi = valid ? nodes[leaf].geom : 0;
  const ptd::Geom* G = geoms + gi;
  f3 pt, nrm;
  const float t = Ar<EX>::template geom_test<TYPE, false>(G, ro, rd, pt, nrm, mk(0.f, 0.f, 0.f));
  keep_closest(&w.best[src], w.rec, src, t, leaf, nrm, pt, valid);
}
// Runs the pending candidates; called at wave-uniform control flow with all 64 lanes active.
// Chunk plan (a typical group at depth >= 1 holds ~55 cubes and ~12 spheres): full chunks of cubes,
// then the remaining cubes together with the spheres in ONE mixed chunk if they fit in 64 lanes
// (costs ~1.3x a pure chunk instead of two pure chunks), otherwise separately.
template <bool CAM, bool EX>
PT_DEV void flush_candidates(const WaveLds& w, int nb, int ns, int lane, f3 o, f3 d,
                             const ptd::Node* __restrict__ nodes, const ptd::Geom* __restrict__ geoms,
                             bool tri) {  // tri (wave-uniform): the back list may hold triangles (mesh extension)
  const int sbase = kCandCap - ns;
  int c0 = 0;
  for (; c0 + 64 <= nb; c0 += 64) run_chunk<1, CAM, EX>(w, c0, 64, 0, 0, lane, o, d, nodes, geoms);
  const int rem = nb - c0;
  if (rem > 0 && ns > 0 && rem + ns <= 64) {
    run_chunk<-1, CAM, EX>(w, c0, rem, sbase, ns, lane, o, d, nodes, geoms);
    return;
  }
  if (rem > 0) run_chunk<1, CAM, EX>(w, c0, rem, 0, 0, lane, o, d, nodes, geoms);
  for (int s0 = 0; s0 < ns; s0 += 64) {
    if (tri) run_chunk<-1, CAM, EX>(w, 0, 0, sbase + s0, min(64, ns - s0), lane, o, d, nodes, geoms);
    else run_chunk<0, CAM, EX>(w, 0, 0, sbase + s0, min(64, ns - s0), lane, o, d, nodes, geoms);
  }
}

// Phase 1 + phase 2 for one group of 64 rays (one per lane; `valid` masks tail lanes).  On return
// w.best[lane] holds the lane's (t bits << 32 | leaf) key (kNoHit if none) and w.rec its normal/point.
template <bool EX>
PT_DEV void trace_group(const WaveLds& w, const float4* top, int ntop, const ptd::Node* __restrict__ nodes,
                        const ptd::Geom* __restrict__ geoms, f3 o, f3 d, bool valid, int lane, float cull,
                        unsigned long long top_xor, bool tri) {
  const RayInv ri = Ar<EX>::ray_inv(d, o);
  w.best[lane] = kNoHit;
  int nb = 0, ns = 0;  // pending cubes (front of the list) / spheres (back)
  uint32_t pend = 0;   // per lane: top entries that are subtrees and whose box this ray passes

  // top list: wave-uniform LDS reads (broadcast), entry e+1 fetched while entry e is tested
  float4 A = top[0], B = top[1];
  for (int e = 0; e < ntop; ++e) {
    const float4 TA = A, TB = B;  // bmin.xyz, bmax.x | bmax.yz, idx, link
    if (e + 1 < ntop) A = top[2 * e + 2], B = top[2 * e + 3];
    const int t_idx = __builtin_amdgcn_readfirstlane(__float_as_int(TB.z));
    const int t_link = __builtin_amdgcn_readfirstlane(__float_as_int(TB.w));
    const bool pass = valid && Ar<EX>::slab(o, ri, TA.x, TA.y, TA.z, TA.w, TB.x, TB.y);
    if (t_link < 0) {  // leaf entry: type is wave-uniform
      const unsigned long long m = ballot(pass);
      if (m) {
        if (nb + ns + 64 > kCandCap) {
          flush_candidates<false, EX>(w, nb, ns, lane, o, d, nodes, geoms, tri);
          nb = ns = 0;
        }
        const int rank = rank_in(m);
        const int cnt = __popcll(m);
        const uint32_t entry = ((uint32_t)t_idx << 6) | (uint32_t)lane;
        if (t_link == -2) {  // cube
          if (pass) w.list[nb + rank] = entry;
          nb += cnt;
        } else {
          if (pass) w.list[kCandCap - ns - cnt + rank] = entry;
          ns += cnt;
        }
      }
    } else if (pass) {
      pend |= 1u << e;
    }
  }
  // (The top-list loop above is restated in carry_search<SUB = true>, which files into the ring: written once, with the leaf filing
  // as a callable, k_intersect and k_features take 12 B / lane of scratch in every build and two instances lose a wave.)
  // subtrees below the cut (the donor table lives in the spare row of w.rec); the chunks fetch the ray from the owner's registers
  scan_subtrees(
      pend, top, o, ri, lane, top_xor, cull, w.best, reinterpret_cast<int*>(w.rec + 6 * 64),
      [&](Walker& wk, bool act, float bt, bool& cand, int& at_n, int& aux) {
        scan_step<EX>(reinterpret_cast<const v4f*>(nodes), wk.o, wk.ri, act, wk.cur, bt, cand, at_n, aux);
      },
      [&](bool cand, int at_n, int own, int aux) {
        const bool cbox = cand && geoms[aux].type == 1;
        const bool csph = cand && !cbox;
        const unsigned long long mb = ballot(cbox), msp = ballot(csph);
        if (mb | msp) {
          if (nb + ns + 128 > kCandCap) {
            flush_candidates<false, EX>(w, nb, ns, lane, o, d, nodes, geoms, tri);
            nb = ns = 0;
          }
          const uint32_t entry = ((uint32_t)at_n << 6) | (uint32_t)own;
          const int rb = rank_in(mb);
          const int rs = rank_in(msp);
          const int cb = __popcll(mb), cs = __popcll(msp);
          if (cbox) w.list[nb + rb] = entry;
          if (csph) w.list[kCandCap - ns - cs + rs] = entry;
          nb += cb;
          ns += cs;
        }
      });
  if (nb + ns) flush_candidates<false, EX>(w, nb, ns, lane, o, d, nodes, geoms, tri);
}

// Primary rays of a scene whose tables stay in memory (more than 32 leaves, no grid): the candidate search as ONE scan of the
// threaded tree for the whole group.  The 64 rays of a group start at the camera and go through neighbouring pixels, so they
// enter nearly the same subtrees: the wave walks the reference's visiting order with wave-uniform node data (scalar loads),
// every lane tests the node's box for its own ray, and a subtree is skipped when NO lane passes its root (the threaded
// `skip` link) — the nodes visited are the union of the lanes' own walks, ~1.5 walks' worth instead of 32 top-list tests plus a
// per-lane scan with work stealing.  Same candidates: a lane files a leaf exactly when its ray passes the leaf's own box, and
// whoever passes that passes every ancestor (exact unions, monotone slab arithmetic), so the lane would have reached it.
typedef __attribute__((address_space(4))) const v4f cnode4;  // wave-uniform indices into it become scalar loads
template <bool EX>
PT_DEV void trace_group_packet(const WaveLds& w, const ptd::Node* __restrict__ nodes, int num_nodes, const ptd::Geom* __restrict__ geoms,
                               f3 o, f3 d, bool valid, int lane, bool tri) {
  const RayInv ri = Ar<EX>::ray_inv(d, o);
  w.best[lane] = kNoHit;
  int nb = 0, ns = 0;  // pending cubes (front of the list) / others (back)
  cnode4* cn = (cnode4*)(uintptr_t)nodes;
  int i = 0;
  // (fetching node i + 1 while node i is tested — the next node whenever some lane passes or a leaf is passed by nobody — was
  // measured: k_primary 1.33 -> 1.39 ms on the 156-primitive scene; the loop is bound by the tests' instructions, not by the loads)
  while (i < num_nodes) {
    const v4f NA = cn[2 * i], NB = cn[2 * i + 1];  // bmin.xyz, bmax.x | bmax.yz, skip, geom
    const bool pass = valid && Ar<EX>::slab(o, ri, NA.x, NA.y, NA.z, NA.w, NB.x, NB.y);
    const unsigned long long m = ballot(pass);
    const int gi = __float_as_int(NB.w);
    if (!m) {
      i = __float_as_int(NB.z);
      continue;
    }
    if (gi >= 0) {  // a leaf some lane passes: type is wave-uniform
      if (nb + ns + 64 > kCandCap) {
        flush_candidates<true, EX>(w, nb, ns, lane, o, d, nodes, geoms, tri);
        nb = ns = 0;
      }
      const int rank = rank_in(m), cnt = __popcll(m);
      const uint32_t entry = ((uint32_t)i << 6) | (uint32_t)lane;
      if (__builtin_amdgcn_readfirstlane(geoms[gi].type) == 1) {
        if (pass) w.list[nb + rank] = entry;
        nb += cnt;
      } else {
        if (pass) w.list[kCandCap - ns - cnt + rank] = entry;
        ns += cnt;
      }
    }
    ++i;
  }
  if (nb + ns) flush_candidates<true, EX>(w, nb, ns, lane, o, d, nodes, geoms, tri);
}

template <bool TABLES_IN_LDS, bool EX>
__global__ __launch_bounds__(kBlock) void k_intersect(SceneTables sc, ptd::Queues qs, const int32_t* __restrict__ cnt_in,
                                                      ptd::PathBuf paths, ptd::HitBuf hits) {
  extern __shared__ float4 lds_raw[];
  char* lds = reinterpret_cast<char*>(lds_raw);
  const IntersectLds L = intersect_lds<TABLES_IN_LDS>(sc);  // [top list][nodes][geoms] (tables, if they fit) then one WaveLds block per wave
  stage16(lds + L.top, EX ? sc.top : sc.top_b, top_bytes(sc));  // EX: primary rays, the reference's arithmetic on the reference's boxes; else the build's bounce tables
  const float4* top = reinterpret_cast<const float4*>(lds + L.top);
  const ptd::Node* nodes = EX ? sc.nodes : sc.nodes_b;
  const ptd::Geom* geoms = sc.geoms;
  if (TABLES_IN_LDS) {
    stage16(lds + L.nodes, nodes, node_bytes(sc));
    stage16(lds + L.geoms, sc.geoms, geom_bytes(sc));
    nodes = reinterpret_cast<const ptd::Node*>(lds + L.nodes);
    geoms = reinterpret_cast<const ptd::Geom*>(lds + L.geoms);
  }
  __syncthreads();
  const int wib = threadIdx.x >> 6;
  WaveLds w = wave_lds_init(lds + L.waves + wib * L.wave_bytes);
  const int ntop = sc.num_top;

  const int wave = blockIdx.x * kWavesPerBlock + wib;
  const int lane = lane_id();
  const auto [q, r, wq] = wave_slot(wave, qs.Q, qs.W);
  const int n_q = cnt_in[cnt_index(qs, 0, q)];
  const int64_t HS = hits.stride;
  const int64_t qbase = (int64_t)q * qs.cap;
  // Memory operations are kept branch-free so that the compiler can count them (s_waitcnt vmcnt(N)
  // is in-order): every lane of a group loads and stores, lanes past the queue's fill level touch the
  // unused tail of the queue's own region (cap is a multiple of 64, so roundup64(n_q) <= cap) and
  // their results are ignored.  The NEXT group's rays are loaded before the current group is traced
  // (software pipeline): their HBM latency overlaps ~1k instructions of work.
  const int last = qs.cap - 64 + lane;  // clamp for the prefetch beyond the last group
  f3 no, nd;
  path_load_ray(paths, qbase + min(r * 64 + lane, last), no, nd);
  for (int j = r; j * 64 < n_q; j += wq) {
    const int i = j * 64 + lane;
    const bool valid = i < n_q;
    const int64_t at = qbase + i;
    const f3 o = no, d = nd;
    path_load_ray(paths, qbase + min((j + wq) * 64 + lane, last), no, nd);
    trace_group<EX>(w, top, ntop, nodes, geoms, o, d, valid, lane, sc.cull_margin, sc.top_xor, sc.has_triangles != 0);

    // record layout of the reference after its per-depth memset (pathtrace.cu:562): miss → t = -1 and zeros elsewhere.
    // (resolve_hit's unpacking, written out with selects: every lane loads and stores, see above — and through resolve_hit's branch
    // the fast build's LDS-table instance takes 82 VGPRs instead of 80 and loses its sixth wave.)
    const unsigned long long best = w.best[lane];
    const bool hit = (uint32_t)(best >> 32) != 0x7f7fffffu;
    const int leaf = hit ? (int)(uint32_t)best : 0;
    hits.t[at] = hit ? __uint_as_float((uint32_t)(best >> 32)) : -1.0f;
    hits.n[at] = hit ? w.rec[0 * 64 + lane] : 0.f;
    hits.n[HS + at] = hit ? w.rec[1 * 64 + lane] : 0.f;
    hits.n[2 * HS + at] = hit ? w.rec[2 * 64 + lane] : 0.f;
    hits.mat[at] = hit ? geoms[nodes[leaf].geom].material : 0;
    hits.p[at] = hit ? w.rec[3 * 64 + lane] : 0.f;
    hits.p[HS + at] = hit ? w.rec[4 * 64 + lane] : 0.f;
    hits.p[2 * HS + at] = hit ? w.rec[5 * 64 + lane] : 0.f;
  }
}

#include "pt_shade.inc"
// ── candidate ring with carry-over (fused kernels) ────────────────────────────────────────
// In the fused kernels the candidates of consecutive groups share one per-wave FIFO ring: a primitive-
// test chunk is run whenever 64 entries are pending, and what is left at the end of a group's search
// (< 64 entries) waits for the next group's candidates instead of being run as a mostly empty chunk.
// A typical depth->=1 group produces ~55 cube + ~12 sphere candidates — one entry too many for one wave —
// so without carry-over every group paid a full cube chunk plus a sphere chunk at ~15 % lane occupancy.
// Entries carry the lane that owns their ray and the parity of their group; the rays themselves (6 floats), like
// the results (closest-hit keys and records), are kept per lane and double-buffered by parity, and a group is shaded one loop iteration later, after every
// entry appended during its search has been processed (forced partial chunk only if the ring never
// filled up in between).  Order of evaluation still does not matter: the (t, leaf) key minimum is the
// reference's choice.
// SMALL: the primary kernel's ring for LDS-table scenes (every leaf is one of <= 32 top entries, so leaf indices are < 64; every
// ray starts at the camera): 16-bit ring entries, no work-stealing table, and only the rays' DIRECTIONS kept — 5888 B per
// wave, which lets a fifth workgroup of k_primary fit a CU.
// NPAR: 2 = keys / records / rays double-buffered by group parity (k_primary's ring: a group is shaded while the next one is
// searched); 1 = one group at a time (k_paths modes 1 and 2, k_primary on the grid).
template <bool SMALL, int NPAR>
struct Carry {
  using Ent = typename std::conditional<SMALL, uint16_t, uint32_t>::type;
  unsigned long long* best;  // [NPAR][64]
  float* rec;                // [NPAR][6][64]  normal xyz, point xyz
  Ent* ent;                  // [kRing]     (leaf << 7) | (parity << 6) | owner lane
  float* ray;                // [NPAR][kRayPlanes][64]  (origin xyz,) direction xyz of each lane's ray, by group parity
  f3 cam_o;                  // SMALL: the origin of every ray (wave-uniform)
  static constexpr int kRayPlanes = SMALL ? 3 : 6;
  int* slot;                 // [64]        scratch of the work-stealing step (carry_search); not SMALL only
  uint32_t* gix;             // [kRing]     LEAN chunks (grid walk) only: geom index | primitive type << 30 of each ring entry
  const float* qo_tab;       // QO chunks (primary rays) only: the camera position in every geom's object space, [geom][3]
  int head, count;           // wave-uniform
  int appended, processed;   // running totals (wave-uniform)
  const __attribute__((address_space(3))) v4f* lnodes;  // the threaded nodes in LDS (k_paths mode 1 on scenes of a few hundred nodes) when lds_nodes
  bool lds_nodes;
};
template <bool SMALL, int NPAR>
PT_DEV Carry<SMALL, NPAR> carry_init(char* base) {  // on a CarryMap<SMALL, NPAR>::bytes block
  using M = CarryMap<SMALL, NPAR>;
  Carry<SMALL, NPAR> c;
  c.best = reinterpret_cast<unsigned long long*>(base + M::best);
  c.rec = reinterpret_cast<float*>(base + M::rec);
  c.ray = reinterpret_cast<float*>(base + M::ray);
  c.ent = reinterpret_cast<typename Carry<SMALL, NPAR>::Ent*>(base + M::ent);
  c.slot = reinterpret_cast<int*>(base + M::slot);
  c.cam_o = mk(0.f, 0.f, 0.f);
  c.head = c.count = c.appended = c.processed = 0;
  c.gix = nullptr;
  c.qo_tab = nullptr;
  c.lnodes = nullptr;
  c.lds_nodes = false;
  return c;
}
// Primitive tests for the first n (<= 64) pending entries; wave-uniform control flow, all lanes active.
// LEAN (the grid walk): the geom index and primitive type come with the ring entry (Carry::gix) instead of through
// nodes[leaf] and the geom record, and the world-space normal is computed for the winner only (finish_normal): 6
// 16-byte reads per candidate instead of 9 (cube) or 11 (sphere) — the L1's access rate is what bounds those kernels.
// QO (the primary kernel's ring): every ray starts at the camera, whose object-space image per geom comes from Carry::qo_tab.
template <bool SMALL, int NPAR, bool EX = false, bool LEAN = false, bool QO = false>
PT_DEV void carry_chunk(Carry<SMALL, NPAR>& c, int n, int lane, const ptd::Node* __restrict__ nodes,
                        const ptd::Geom* __restrict__ geoms) {
  const bool valid = lane < n;
  PT_STAT(6, 1);
  PT_STAT(7, n);
  const int idx = (c.head + lane) & (kRing - 1);
  const uint32_t entry = (uint32_t)c.ent[idx];
  const int src = (int)(entry & 63u);
  const int par = (int)((entry >> 6) & 1u);
  const uint32_t leaf = entry >> 7;
  constexpr int RP = Carry<SMALL, NPAR>::kRayPlanes;
  const float* ray = c.ray + par * RP * 64 + src;
  const f3 ro = SMALL ? c.cam_o : mk(ray[0 * 64], ray[1 * 64], ray[2 * 64]);
  const f3 rd = mk(ray[(RP - 3) * 64], ray[(RP - 2) * 64], ray[(RP - 1) * 64]);
  const uint32_t gw = LEAN ? c.gix[idx] : 0u;
  const int gi = valid ? (LEAN ? (int)(gw & 0x3fffffffu) : nodes[leaf].geom) : 0;
  const ptd::Geom* G = geoms + gi;
  f3 pt = mk(0.f, 0.f, 0.f), nrm = mk(0.f, 0.f, 0.f);
  float t = -1.0f;
  // cube / sphere decided per lane; shared pre and post parts
  if (LEAN) t = Ar<EX>::template geom_test<-1, false, true>(G, ro, rd, pt, nrm, mk(0.f, 0.f, 0.f), valid ? (int)(gw >> 30) : 0);
  else if (QO) t = Ar<EX>::template geom_test<-1, true>(G, ro, rd, pt, nrm, mk(c.qo_tab[3 * gi], c.qo_tab[3 * gi + 1], c.qo_tab[3 * gi + 2]));
  else t = Ar<EX>::template geom_test<-1, false>(G, ro, rd, pt, nrm, mk(0.f, 0.f, 0.f));
  keep_closest(&c.best[par * 64 + src], c.rec + par * 6 * 64 + src, 0, t, leaf, nrm, pt, valid);
  c.head = (c.head + n) & (kRing - 1);
  c.count -= n;
  c.processed += n;
}
// Append the lanes with `pass` (entry: leaf index, group parity, lane that owns the ray); runs a chunk as soon
// as 64 entries are pending.  Wave-uniform control flow.
template <bool SMALL, int NPAR, bool EX = false, bool LEAN = false>
PT_DEV void carry_append(Carry<SMALL, NPAR>& c, bool pass, uint32_t leaf, int par, int owner, int lane,
                         const ptd::Node* __restrict__ nodes, const ptd::Geom* __restrict__ geoms, uint32_t gword = 0u) {
  const unsigned long long m = ballot(pass);
  if (!m) return;
  const int rank = rank_in(m);
  if (pass) {
    const int idx = (c.head + c.count + rank) & (kRing - 1);
    c.ent[idx] = (typename Carry<SMALL, NPAR>::Ent)((leaf << 7) | ((uint32_t)par << 6) | (uint32_t)owner);
    if (LEAN) c.gix[idx] = gword;
  }
  const int cnt = __popcll(m);
  c.count += cnt;
  c.appended += cnt;
  if (c.count >= 64) carry_chunk<SMALL, NPAR, EX, LEAN>(c, 64, lane, nodes, geoms);
}
// Candidate search of one group (phase 1 of trace_group) feeding the ring.
// SUB: the scene has subtrees below the top list.  The LDS-table kernels are only used for scenes whose leaves all
// fit the top list (lds_table_limit), so their instantiation drops the subtree scan.
// CAM (primary rays, !SUB only): `top` holds the boxes relative to the camera position (slab_rel), EX selects the
// reference's exact arithmetic, and the chunks take the object-space origin from Carry::qo_tab.
template <bool SUB, int NPAR, bool CAM = false, bool EX = false>
PT_DEV void carry_search(Carry<!SUB, NPAR>& c, const float4* top, int ntop, const ptd::Node* __restrict__ nodes,
                         const ptd::Geom* __restrict__ geoms, f3 o, f3 d, bool valid, int lane, int par, float cull,
                         unsigned long long top_xor) {
  static_assert(CAM == !SUB, "the top-list-only form is the primary kernel's camera ring (Carry<true>: origins not stored); subtree scans take any origin");
  const RayInv ri = Ar<EX>::ray_inv(d, o);
  {
    constexpr int RP = Carry<!SUB, NPAR>::kRayPlanes;
    float* ray = c.ray + par * RP * 64 + lane;  // this group's rays, read back by the primitive-test chunks
    if (RP == 6) ray[0 * 64] = o.x, ray[1 * 64] = o.y, ray[2 * 64] = o.z;
    ray[(RP - 3) * 64] = d.x, ray[(RP - 2) * 64] = d.y, ray[(RP - 1) * 64] = d.z;
  }
  if (!SUB) {
    // Every top entry is a leaf (the LDS-table kernels): first all box tests — one bit per entry in a per-lane mask, boxes
    // fetched one entry ahead into alternating registers (unrolled by two, no copies) — then the appends lane-major: in
    // round j every lane that still has candidates files one, so the ballot / rank / ring arithmetic runs once per round
    // (max candidates of a lane, ~3) instead of once per entry (7 for cornell.txt).  The order of the ring entries changes,
    // the set does not, and the closest-hit key is order-independent.
    // box tests, eight at a time fully unrolled (no loop-carried box registers to rotate); the pass bit is shifted into the mask
    // by ONE v_addc (push_bit): bit (ntop - 1 - e) of the mask = entry e.  (paths_search restates this two-phase search.)
    uint32_t mask = 0;
    for (int e0 = 0; e0 < ntop; e0 += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + u;
        if (e < ntop) {
          const float4 A = top[2 * e], B = top[2 * e + 1];
          mask = push_bit(mask, CAM ? Ar<EX>::slab_rel(ri, A.x, A.y, A.z, A.w, B.x, B.y) : Ar<EX>::slab(o, ri, A.x, A.y, A.z, A.w, B.x, B.y));
        }
      }
    }
    mask = valid ? mask : 0u;
    const uint32_t tag = ((uint32_t)par << 6) | (uint32_t)lane;
    while (true) {
      const unsigned long long m = ballot(mask != 0u);
      if (!m) break;
      const int rank = rank_in(m);
      if (mask != 0u) {
        const int te = ntop - 1 - __builtin_ctz(mask);
        mask &= mask - 1u;
        const uint32_t leaf = __float_as_uint(reinterpret_cast<const float*>(top)[8 * te + 6]);  // TopEntry::idx
        c.ent[(c.head + c.count + rank) & (kRing - 1)] = (typename Carry<!SUB, NPAR>::Ent)((leaf << 7) | tag);
      }
      const int cnt = __popcll(m);
      c.count += cnt;
      c.appended += cnt;
      if (c.count >= 64) carry_chunk<!SUB, NPAR, EX, false, CAM>(c, 64, lane, nodes, geoms);
    }
    return;
  }
  // (The top-list loop below restates trace_group's, which files into the two-ended list.)
  uint32_t pend = 0;  // per lane: top entries that are subtrees and whose box this ray passes
  PT_STAT(0, 1);
  PT_STAT(13, __popcll(ballot(valid)));
  float4 A = top[0], B = top[1];
  for (int e = 0; e < ntop; ++e) {
    const float4 TA = A, TB = B;  // bmin.xyz, bmax.x | bmax.yz, idx, link
    if (e + 1 < ntop) A = top[2 * e + 2], B = top[2 * e + 3];
    const int t_idx = __builtin_amdgcn_readfirstlane(__float_as_int(TB.z));
    const int t_link = __builtin_amdgcn_readfirstlane(__float_as_int(TB.w));
    const bool pass = valid && slab(o, ri, TA.x, TA.y, TA.z, TA.w, TB.x, TB.y);
    PT_STAT(8, __popcll(ballot(pass)));
    // (the closer-hit cull on top entries that are leaves — scenes of a few dozen primitives, where all of them are — was measured:
    // 32 primitives 9.9 -> 9.2 k Msamples/s; the list is not in near-first order and every entry pays the LDS read of the best hit)
    if (t_link < 0) carry_append(c, pass, (uint32_t)t_idx, par, lane, lane, nodes, geoms);
    else if (pass) pend |= 1u << e;
  }
  // Subtrees below the cut (large scenes only): per-lane stackless scans, nearest subtree first, with work stealing
  // (scan_step / steal_step); candidates are filed under the lane that owns the ray, so nothing downstream changes.
  if constexpr (SUB)
    scan_subtrees(
        pend, top, o, ri, lane, top_xor, cull, c.best + par * 64, c.slot,
        [&](Walker& wk, bool act, float bt, bool& cand, int& at_n, int& aux) {
          if (c.lds_nodes) scan_step(c.lnodes, wk.o, wk.ri, act, wk.cur, bt, cand, at_n, aux);
          else scan_step(reinterpret_cast<const v4f*>(nodes), wk.o, wk.ri, act, wk.cur, bt, cand, at_n, aux);
        },
        [&](bool cand, int at_n, int own, int) { carry_append(c, cand, (uint32_t)at_n, par, own, lane, nodes, geoms); });
}
// Make sure everything appended up to `mark` has been tested (only runs a partial chunk when the ring
// did not fill up since).
template <bool SMALL, int NPAR, bool EX = false, bool QO = false>
PT_DEV void carry_drain_to(Carry<SMALL, NPAR>& c, int mark, int lane, const ptd::Node* __restrict__ nodes,
                           const ptd::Geom* __restrict__ geoms) {
  while (c.processed - mark < 0) carry_chunk<SMALL, NPAR, EX, false, QO>(c, min(64, c.count), lane, nodes, geoms);
}

#include "pt_grid.inc"
// k_intersect's stage form of the grid walk (tests: pt_stage_intersect_grid hands it rays no camera produces): k_intersect's
// queue, group and prefetch frame around the per-group body of the fused kernels on a grid — grid_search, the drain of the
// candidate ring, the winner's normal — with nothing of its own in between.  EX = kD0: the depth-0 form (k_primary: the
// reference's arithmetic on grid_items, without the near_scene pre-test, which is no part of the walk); EX = false: the
// bounce form (k_paths<kGrid>: the build's arithmetic on grid_items_b).  Stands here, not beside k_intersect: after the walk.
template <bool EX>
__global__ __launch_bounds__(kBlock) void k_intersect_grid(SceneTables sc, ptd::Queues qs, const int32_t* __restrict__ cnt_in,
                                                           ptd::PathBuf paths, ptd::HitBuf hits) {
  extern __shared__ float4 lds_raw[];
  char* lds = reinterpret_cast<char*>(lds_raw);
  const IntersectGridLds L = intersect_grid_lds<kFast, EX>(sc);  // one grid block per wave; the tables stay in memory
  const ptd::Node* nodes = EX ? sc.nodes : sc.nodes_b;
  const ptd::Geom* geoms = sc.geoms;
  const int wib = threadIdx.x >> 6;
  GridRings ws = grid_rings_init<EX>(lds + L.waves + wib * L.wave_bytes);
  const LeafGeom<true, EX> leaf_geom{nodes, geoms};  // the grid's chunks leave the normal to the winner

  const int wave = blockIdx.x * kWavesPerBlock + wib;
  const int lane = lane_id();
  const auto [q, r, wq] = wave_slot(wave, qs.Q, qs.W);
  const int n_q = cnt_in[cnt_index(qs, 0, q)];
  const int64_t HS = hits.stride;
  const int64_t qbase = (int64_t)q * qs.cap;
  // (k_intersect's frame: lanes past the fill level trace nothing and store a miss into the unused tail of the queue's region)
  const int last = qs.cap - 64 + lane;
  f3 no, nd;
  path_load_ray(paths, qbase + min(r * 64 + lane, last), no, nd);
  for (int j = r; j * 64 < n_q; j += wq) {
    const int i = j * 64 + lane;
    const bool valid = i < n_q;
    const int64_t at = qbase + i;
    const f3 o = no, d = nd;
    path_load_ray(paths, qbase + min((j + wq) * 64 + lane, last), no, nd);
    ws.cy.best[lane] = kNoHit;
    grid_search<1, EX>(ws.cy, ws.cr, sc, nodes, geoms, o, d, valid, lane, 0);
    while (ws.cy.count > 0) carry_chunk<false, 1, EX, true>(ws.cy, min(64, ws.cy.count), lane, nodes, geoms);
    const Hit h = resolve_hit(ws.cy.best[lane], ws.cy.rec + lane, valid, leaf_geom);  // a miss: t = -1, zeros elsewhere
    hits.t[at] = h.t;
    hits.n[at] = h.n.x, hits.n[HS + at] = h.n.y, hits.n[2 * HS + at] = h.n.z;
    hits.mat[at] = h.mat;
    hits.p[at] = h.p.x, hits.p[HS + at] = h.p.y, hits.p[2 * HS + at] = h.p.z;
  }
}
// Waves per SIMD a k_primary instance is compiled for.  Two shared instances end at 72 VGPRs — seven waves, which the persistent
// grid of a scene with little LDS per block uses — by the allocator's choice, not by the bound; their SPLIT forms came out at 74
// under the same bound and are asked for the seven outright (72 VGPRs, no scratch; exact / kTopScan would spill, and has six either way).
template <Search F, int SPLIT>
constexpr int primary_waves() {
  return SPLIT == kSplitRecords && ((PT_ARITH == 2 && F == kTopScan) || (PT_ARITH == 0 && F == kLdsTables)) ? 7 : kPrimaryWaves;
}
// ── depth 0 fused: generateRayFromCamera + computeIntersections + shadeAndExtendRays ────────
// Primary rays are a pure function of the sample id, so depth 0 needs no path state in memory at
// all: the ray is built in registers, traced with the same wave-cooperative search, shaded, and
// only its outcome is written — the survivor's new ray into the depth-1 queues or the retired
// colour.  That removes the generate launch and ~190 B/sample of HBM round trips (40 B ray state
// written + 24 B read, 32 B hit record written + read, 28 B path state re-read) at the one depth
// where every sample is alive.  Also writes the per-queue sample counts of depth 0 (statistics).
// kGrid: large scenes with a uniform grid over the leaf boxes (SceneTables::use_grid): the primary rays walk it like the
// bounce rays do (grid_search) instead of testing the top list and scanning subtrees; exact arithmetic as in every depth-0 path.
// kLdsTables (e.g. cornell.txt): the candidates go through the bounce kernel's ring with carry-over
// (carry_search / carry_chunk), so that primitive tests only ever run as full 64-entry chunks — a group of primary rays
// files ~85 candidates, which the per-group form (trace_group) ran as one full chunk plus one a third full — and the
// appends run lane-major (two-phase search).  A group is shaded one loop iteration after its search.
// Unlike the ring form tried in round 2 it keeps the camera-relative boxes and the per-geom object-space camera position.
// kTopScan (tables in memory, no grid): one wave-uniform scan of the threaded tree per group (trace_group_packet) instead of
// top list + per-lane subtree scans.
// SHARE (BatchInfo::primary_share > 1, no aa_jitter, not flat; pt_sched.h): the camera ray of a pixel, and so its hit key, normal
// and point, do not depend on the iteration — the loop nest is chunk outer, iteration inner: a chunk is generated, searched and
// resolved ONCE per run of iterations and shaded in each of them with that iteration's seed (every sample is still drawn, shaded,
// bounced and stored; the records, their order and the image are those of the per-iteration form, which stays for jittered
// rays, the flat lists and as the A/B switch PtOptions.debug_flags 128).  The search sits above the shading in all three forms.
// BatchInfo::retire_once (pt_sched.h): the records of the lanes that retire here — the same lanes with the same colour in every
// iteration — are stored in iteration 0 of the batch only, and a group that holds nothing else skips the iteration loop.
// SPLIT (BatchInfo::split_records, shared form only; pt_sched.h): a survivor's record is the 16-byte per-iteration word (direction,
// sample id | specular bit) in plane 0 and, from the run that holds iteration 0 of the batch only, the 16-byte invariant word
// (origin, material index) in plane 1 at the slot of iteration 0; its throughput is not stored at all.
// SPLIT == kFirstBounce (BatchInfo::split_records 2, kLdsTables only; pt_sched.h batch_form): the kernel has no per-iteration work
// left — a chunk is traced once per BATCH, a survivor's one record (bounce origin, hit normal, camera direction, pixel | material)
// goes to the slot of iteration 0, and k_paths decides depth 0 and samples the first bounce of every iteration from it.
template <Search F, bool SHARE = false, int SPLIT = 0>
__global__ __launch_bounds__(kBlock, (primary_waves<F, SPLIT>())) void k_primary(SceneTables sc, ptd::Camera cam, BatchInfo b, ptd::Queues qs,
                                                    int32_t* __restrict__ cnt0, int32_t* __restrict__ cnt_out,
                                                    ptd::PathBuf out, ptd::RetireBuf ret) {
  extern __shared__ float4 lds_raw[];
  char* lds = reinterpret_cast<char*>(lds_raw);
  constexpr bool GRID = F == kGrid, TABLES_IN_LDS = F == kLdsTables, RING = TABLES_IN_LDS;
  const PrimaryLds L = primary_lds<F, kFast, kD0>(sc);
  stage16(lds + L.top, sc.top, GRID ? 0 : top_bytes(sc));
  stage16(lds + L.mats, sc.mats, mat_bytes(sc));
  const ptd::Mat* mats = reinterpret_cast<const ptd::Mat*>(lds + L.mats);
  const ptd::Node* nodes = sc.nodes;
  const ptd::Geom* geoms = sc.geoms;
  if (TABLES_IN_LDS) {
    stage16(lds + L.nodes, sc.nodes, node_bytes(sc));
    stage16(lds + L.geoms, sc.geoms, geom_bytes(sc));
    nodes = reinterpret_cast<const ptd::Node*>(lds + L.nodes);
    geoms = reinterpret_cast<const ptd::Geom*>(lds + L.geoms);
  }
  uint32_t* ihash = reinterpret_cast<uint32_t*>(lds + L.ihash);
  iter_hash_fill(ihash, sc, b, 0);
  // camera-relative copies for the primary rays: top-list boxes minus the camera position and (tables in LDS only)
  // the camera position in each geom's object space — the same float operations the per-ray code would execute
  float4* cam_top = reinterpret_cast<float4*>(lds + L.cam_top);
  float* cam_qo = reinterpret_cast<float*>(lds + L.cam_qo);
  {
    const f3 cp = mk(cam.pos[0], cam.pos[1], cam.pos[2]);
    for (int e = threadIdx.x; !GRID && e < sc.num_top; e += blockDim.x) {
      const ptd::TopEntry t = sc.top[e];
      cam_top[2 * e] = make_float4(t.bmin[0] - cp.x, t.bmin[1] - cp.y, t.bmin[2] - cp.z, t.bmax[0] - cp.x);
      cam_top[2 * e + 1] = make_float4(t.bmax[1] - cp.y, t.bmax[2] - cp.z, __int_as_float(t.idx), __int_as_float(t.link));
    }
    for (int gi = threadIdx.x; TABLES_IN_LDS && gi < sc.num_geoms; gi += blockDim.x) {
      const f3 q = Ar<kD0>::xf_point(sc.geoms[gi].inv, cp);
      cam_qo[3 * gi] = q.x, cam_qo[3 * gi + 1] = q.y, cam_qo[3 * gi + 2] = q.z;
    }
  }
  __syncthreads();
  const int wib = threadIdx.x >> 6;
  // the form's per-wave state: the camera ring (kLdsTables), the bounce kernel's rings (kGrid) or one group's candidate list
  char* wbase = lds + L.waves + wib * L.wave_bytes;
  auto ws = [wbase] {
    if constexpr (RING) return carry_init<true, 2>(wbase);
    else if constexpr (GRID) return grid_rings_init<kD0>(wbase);
    else return wave_lds_init(wbase);
  }();
  const int ntop = sc.num_top;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + wib);  // (the compiler cannot see that threadIdx.x >> 6 is wave-uniform)
  const int lane = lane_id();
  // A strand = what one wave of one queue traces at depth 0: in iteration k the queue's chunks of residue (r + k) mod wq.  Wave w
  // runs strand w.  With a small tile (a rank's share of a frame: a queue owns a dozen chunks, some of them beside the scene,
  // which cost a bounds test) the strands differ by +-20 %: they are then cut into `pieces` runs of iterations — every
  // (queue, iteration, residue) still has ONE owner, which is all the sub-lists ask for — piece 0 stays with wave w and the
  // others go to whoever is free, in the order of a counter (zeroed by k_count_stats).
  const StrandPlan plan = strand_plan(b.K, b.primary_pieces, qs.deal != nullptr, b.flat != 0);
  for (int strand = wave; strand < qs.W * plan.pieces;) {
    const Strand st = strand_of(strand, plan, b.K, qs.Q, qs.W);
    const int piece = st.piece, q = st.q, r = st.r, wq = st.wq, k0 = st.k0, k1 = st.k1;  // (lambdas below capture them)
    const Retire rt = retire_of(ret, q);
    // The wave's samples: in iteration k the chunks jj = rho, rho + wq, ... of the queue's my_nq (chunk jj = tile chunk q + jj * Q),
    // rho = (r + k) mod wq — its own sub-list and sub-region of (q, k) (pt_device.h RetireBuf): positions come from the two
    // counters below, nothing is reserved with atomics and every store is issued where its group is shaded.
    const QueueShare sh = queue_share(b, qs, q);
    if (piece == 0 && r == 0 && lane == 0) cnt0[cnt_index(qs, 0, q)] = b.K * sh.my_pixels;
    const int64_t qbase = (int64_t)q * qs.cap;
    const float inv_w = 1.0f / (float)cam.res_x;
    const f3 o = mk(cam.pos[0], cam.pos[1], cam.pos[2]);
    int32_t* counter = &cnt_out[cnt_index(qs, 0, q)];  // flat form: the queue's ONE depth-1 list
    const int quo = sh.my_nq / wq, rem = sh.my_nq % wq;
    int ck = k0 - 1, crho = strand_rho_before(r, k0, wq), nl = 0, nd = 0;  // iteration the counters belong to, its residue (r + ck) mod wq; survivors / retirees of the wave in it so far
    auto publish = [&]() {  // the finished iteration's counts (also when the wave had no chunk in it: zeros)
      if (ck >= k0 && lane == 0) rt.sub[ck * rt.wq0 + crho] = ((unsigned long long)(uint32_t)nd << 32) | (uint32_t)nl;
    };
    auto next_iteration = [&]() {  // publish, then on to ck + 1
      publish();
      nl = nd = 0;
      ++ck;
      crho = crho + 1 == wq ? 0 : crho + 1;
    };
    // A group of 64 primary rays (one per lane): what its shading needs besides the hit.  (valid is an int: as a bool the exact
    // build's two shared ring instances lose their seventh wave — 74 VGPRs, or 20 B / lane of scratch under the bound.)
    struct Group {
      f3 d;
      int k, pl, slot;  // pl: tile pixel; k, slot (per-iteration form only): the iteration inside the batch and the sample id
      uint32_t phash;
      int valid;  // 0: a lane past the tile's last pixel
    };
    // generate: chunk jj of the queue (in iteration k: the shared form's rays do not depend on it and pass 0)
    auto group_of = [&](int jj, int k) {
      Group g;
      const int pl_raw = chunk_pixel(q, jj, qs.Q) + lane;
      g.valid = pl_raw < b.N;
      g.pl = g.valid ? pl_raw : b.N - 1;
      g.k = k, g.slot = SHARE ? 0 : make_slot(b, k, g.pl);
      const int p = global_pixel(b, g.pl);  // global pixel index
      g.phash = utilhash((uint32_t)p);
      float jx = 0.f, jy = 0.f;
      const bool aa = !SHARE && b.aa_jitter != 0;  // (the shared form is chosen for unjittered rays only)
      if (aa) aa_jitter(b.iter_first + k, p, jx, jy);
      g.d = Ar<kD0>::camera_dir(cam, inv_w, p, aa, jx, jy);
      return g;
    };
    // the group that waits between its search and its shading (RING: shaded one group later)
    struct {
      Group g;
      int par, mark;
      bool any;
    } pp;
    pp.any = false;
    // Search of group `g`, the `it`-th of the wave's loop, then shade(key, record column, group) of the group whose hit is resolved
    // by then: g itself, or in the ring form the group before it — the last one is left to the loop's end (the tails below).
    auto trace = [&](int it, const Group& g, auto&& shade) {
      // Primary rays come in bundles of 64 neighbouring pixels and half of the 16:9 frame looks past the scene:
      // one test against the bounds of the whole tree per lane, and if no lane passes (a parent box rejects
      // whatever its children would, the slab arithmetic being monotone) the 7 leaf-box tests are skipped.
      const bool near_scene = ballot(g.valid && Ar<kD0>::slab(o, Ar<kD0>::ray_inv(g.d, o), sc.root_min[0], sc.root_min[1], sc.root_min[2],
                                                       sc.root_max[0], sc.root_max[1], sc.root_max[2])) != 0;
      if constexpr (RING) {
        const int par = it & 1;
        ws.best[par * 64 + lane] = kNoHit;
        if (near_scene) carry_search<false, 2, true, kD0>(ws, cam_top, ntop, nodes, geoms, o, g.d, g.valid, lane, par, sc.cull_margin, sc.top_xor);
        if (pp.any) {  // the waiting group's candidates are now all resolved; its key and record stay in its parity's half while it is shaded
          carry_drain_to<true, 2, kD0, true>(ws, pp.mark, lane, nodes, geoms);
          shade(ws.best[pp.par * 64 + lane], ws.rec + pp.par * 6 * 64 + lane, pp.g);
        }
        pp.g = g, pp.par = par, pp.mark = ws.appended, pp.any = true;
      } else if constexpr (GRID) {
        ws.cy.best[lane] = kNoHit;
        if (near_scene) {
          grid_search<1, kD0>(ws.cy, ws.cr, sc, nodes, geoms, o, g.d, g.valid, lane, 0);
          while (ws.cy.count > 0) carry_chunk<false, 1, kD0, true>(ws.cy, min(64, ws.cy.count), lane, nodes, geoms);
        }
        shade(ws.cy.best[lane], ws.cy.rec + lane, g);
      } else {
        if (near_scene) trace_group_packet<kD0>(ws, nodes, sc.num_nodes, geoms, o, g.d, g.valid, lane, sc.has_triangles != 0);
        else ws.best[lane] = kNoHit;
        shade(ws.best[lane], ws.rec + lane, g);
      }
    };
    const LeafGeom<GRID, kD0> leaf_geom{nodes, geoms};  // the grid's chunks leave the normal to the winner
    // shading + retirement + compaction of one group of primary rays from its resolved hit key / record
    auto shade_group = [&](unsigned long long best, const float* rec, const Group& g) {
      const bool valid = g.valid;
      const int k = g.k, pl = g.pl;
      ShadeIO s;
      s.o = o;
      s.d = g.d;
      s.c = mk(1.0f, 1.0f, 1.0f);
      s.alive = false;
      Bounce bo;
      bo.kind = 0;
      const Hit h = resolve_hit(best, rec, valid, leaf_geom);
      if (valid) bo = shade_decide(mats, b.trace_depth, 0, iter_hash_of(ihash, sc, b, 0, k) ^ g.phash, h.t, h.mat, s);
      const bool alive = valid && s.alive, dead = valid && !s.alive;
      if (alive) shade_bounce(bo, h.n, h.p, s);
      const unsigned long long live = ballot(alive);
      const PathTag tag{g.slot, g.phash, k};
      if (b.flat) {  // unfused consumers: one dense list per queue behind an atomic, records appended one by one (test / A-B form)
        int base = 0;
        if (live && lane == 0) base = atomicAdd(counter, (int)__popcll(live));
        base = __builtin_amdgcn_readfirstlane(base);
        if (alive) path_store(out, qbase + base + rank_in(live), s.o, s.d, s.c, tag);
        retire_append(rt, dead, k, pl, s.c);
        return;
      }
      while (ck < k) next_iteration();  // first group of a new iteration: the previous one's counts are final (iterations without a chunk publish zeros on the way)
      const int sub0 = k * rt.seg_cap + sub_offset(quo, rem, crho) * 64;  // first slot of sub-list / sub-region (q, k, rho)
      const unsigned long long deadm = ballot(dead);
      if (alive) path_store(out, qbase + sub0 + nl + rank_in(live), s.o, s.d, s.c, tag);
      if (dead) rt.rec[sub0 + nd + rank_in(deadm)] = ptd::Word4{s.c.x, s.c.y, s.c.z, __int_as_float(pl)};
      nl += (int)__popcll(live), nd += (int)__popcll(deadm);
    };
    if constexpr (RING) ws = carry_init<true, 2>(wbase), ws.qo_tab = cam_qo, ws.cam_o = o;  // every strand starts with an empty ring
    if constexpr (SHARE && SPLIT == kFirstBounce) {
      // First bounce in k_paths (pt_sched.h batch_form; the host gives such a batch ONE piece, and the run is the whole batch):
      // chunk jj is traced once, a surviving pixel gets its one record — what every iteration's depth-0 shading starts from — at the
      // slot of iteration 0, a retiring one its record as in every BatchInfo::retire_once batch, and the pair of counts, the same in
      // every iteration, goes to sub[] of all of them.  No iteration loop, no shade_decide of a survivor, no direction sampling.
      const int sub_off = sub_offset(quo, rem, shared_rho(r, 0, wq)) * 64;
      int fnl = 0, fnd = 0;  // survivors / retirees of the wave's chunks so far (wave-uniform)
      auto record_group = [&](unsigned long long best, const float* rec, const Group& g) {
        const bool valid = g.valid;
        const Hit h = resolve_hit(best, rec, valid, leaf_geom);
        const bool cdead = valid && (h.t < 0.0f || mats[h.mat].emittance > 0.0f), lives = valid && !cdead;  // shade_decide's own tests (see retire_once below)
        const unsigned long long livem = ballot(lives), cdeadm = ballot(cdead);
        if (lives) path_store(out, qbase + sub_off + fnl + rank_in(livem), bounce_origin(h.n, h.p), h.n, g.d, PathTag{pack_first(g.pl, h.mat, b.slot_shift), g.phash, 0});
        if (cdead) {
          ShadeIO s;
          s.o = o;
          s.d = g.d;
          s.c = mk(1.0f, 1.0f, 1.0f);
          s.alive = false;
          shade_decide(mats, b.trace_depth, 0, iter_hash_of(ihash, sc, b, 0, 0) ^ g.phash, h.t, h.mat, s);
          rt.rec[sub_off + fnd + rank_in(cdeadm)] = ptd::Word4{s.c.x, s.c.y, s.c.z, __int_as_float(g.pl)};
        }
        fnl += (int)__popcll(livem), fnd += (int)__popcll(cdeadm);
      };
      pp.any = false;
      int it = 0;
      for (int jj = shared_rho(r, 0, wq); jj < sh.my_nq; jj += wq, ++it) trace(it, group_of(jj, 0), record_group);
      if constexpr (RING) {  // the ring's last group (see the shared form's tail)
        if (pp.any) {
          carry_drain_to<true, 2, kD0, true>(ws, pp.mark, lane, nodes, geoms);
          record_group(ws.best[pp.par * 64 + lane], ws.rec + pp.par * 6 * 64 + lane, pp.g);
        }
      }
      // identical counts (zeros where the wave had no chunk) for every iteration the regions are provisioned for, not this batch's K
      // alone: a longer batch of the same camera finds them without another trace (pt_sched.h batch_form); kmax may exceed the 64 lanes
      for (int k = lane; k < ret.kmax; k += 64) rt.sub[k * rt.wq0 + shared_rho(r, k, wq)] = ((unsigned long long)(uint32_t)fnd << 32) | (uint32_t)fnl;
    } else if constexpr (SHARE) {
      // Shared form (pt_sched.h): the wave keeps residue r through the piece, so chunk jj is traced ONCE per run of iterations
      // [s0, s1) and shaded s1 - s0 times from the same hit; lane l of vnl / vnd counts the survivors / retirees of iteration s0 + l.
      const int cap = shared_run_cap(b.primary_share), sub_off = sub_offset(quo, rem, shared_rho(r, k0, wq)) * 64;
      const bool once = b.retire_once != 0;
      for (int run = 0, runs = shared_runs(k0, k1, cap); run < runs; ++run) {
        const Run sr = shared_run(k0, k1, cap, run);
        const int s0 = sr.k0, s1 = sr.k1;
        int vnl = 0, vnd = 0;
        // shading + retirement + compaction of one group of primary rays in every iteration of the run
        auto shade_run = [&](unsigned long long best, const float* rec, const Group& g) {
          const bool valid = g.valid;
          const int pl = g.pl;
          const uint32_t phash = g.phash;
          const f3 d = g.d;
          const Hit h = resolve_hit(best, rec, valid, leaf_geom);
          const float ht = h.t;
          const int hmat = h.mat;
          const f3 hn = h.n, hp = h.p;
          if constexpr (SPLIT == kSplitRecords) {
            // BatchInfo::split_records (pt_sched.h): the lanes that survive — every hit but an emitter's, in every iteration — get their
            // invariant word (shade_bounce's origin, the material) from the run that holds iteration 0 of the batch, at the slot their
            // records have in that iteration (invariant_slot of every other iteration's).
            if (s0 == 0) {
              const bool lives = valid && !(ht < 0.0f || mats[hmat].emittance > 0.0f);
              const unsigned long long livem = ballot(lives);
              const f3 o1 = bounce_origin(hn, hp);
              if (lives) out.r[out.stride + qbase + sub_off + __builtin_amdgcn_readlane(vnl, 0) + rank_in(livem)] = ptd::Word4{o1.x, o1.y, o1.z, __int_as_float(hmat)};
            }
          }
          // BatchInfo::retire_once (pt_sched.h): a miss or an emitter hit retires here in every iteration with the same colour — the
          // tests are shade_decide's own, which returns for both before it uses a draw — and every other hit survives.  Those lanes'
          // records are written in iteration 0 of the batch only, to the slots they have always had; vnd still advances in every
          // iteration, so sub[], k_paths' slots and the statistics are what they were.
          const bool cdead = once && valid && (ht < 0.0f || mats[hmat].emittance > 0.0f);
          const unsigned long long cdeadm = once ? ballot(cdead) : 0ull;
          if (once) {
            if (s0 == 0 && cdeadm) {  // this run holds iteration 0 of the batch
              ShadeIO s;
              s.o = o;
              s.d = d;
              s.c = mk(1.0f, 1.0f, 1.0f);
              s.alive = false;
              if (cdead) {
                shade_decide(mats, b.trace_depth, 0, iter_hash_of(ihash, sc, b, 0, 0) ^ phash, ht, hmat, s);
                rt.rec[sub_off + __builtin_amdgcn_readlane(vnd, 0) + rank_in(cdeadm)] = ptd::Word4{s.c.x, s.c.y, s.c.z, __int_as_float(pl)};
              }
            }
            if (ballot(valid && !cdead) == 0) {  // nobody survives, in any iteration: only the counts move
              if (lane < s1 - s0) vnd += (int)__popcll(cdeadm);
              return;
            }
          }
          for (int k = s0; k < s1; ++k) {
            ShadeIO s;
            s.o = o;
            s.d = d;
            s.c = mk(1.0f, 1.0f, 1.0f);
            s.alive = false;
            Bounce bo;
            bo.kind = 0;
            if (valid) bo = shade_decide(mats, b.trace_depth, 0, iter_hash_of(ihash, sc, b, 0, k) ^ phash, ht, hmat, s);
            const bool alive = valid && s.alive, dead = valid && !s.alive;
            if (alive) shade_bounce(bo, hn, hp, s);
            const unsigned long long live = ballot(alive), deadm = once ? cdeadm : ballot(dead);
            const int nl = __builtin_amdgcn_readlane(vnl, k - s0), nd = __builtin_amdgcn_readlane(vnd, k - s0);
            const int sub0 = k * rt.seg_cap + sub_off;  // first slot of sub-list / sub-region (q, k, r)
            const PathTag tag{make_slot(b, k, pl), phash, k};
            if constexpr (SPLIT == kSplitRecords) {
              if (alive) out.r[qbase + sub0 + nl + rank_in(live)] = ptd::Word4{s.d.x, s.d.y, s.d.z, __uint_as_float(pack_kind(tag.slot, bo.kind == 1))};
            } else if (alive) path_store(out, qbase + sub0 + nl + rank_in(live), s.o, s.d, s.c, tag);
            if (dead && !once) rt.rec[sub0 + nd + rank_in(deadm)] = ptd::Word4{s.c.x, s.c.y, s.c.z, __int_as_float(pl)};
            if (lane == k - s0) vnl += (int)__popcll(live), vnd += (int)__popcll(deadm);
          }
        };
        if constexpr (RING) ws = carry_init<true, 2>(wbase), ws.qo_tab = cam_qo, ws.cam_o = o;  // every run starts with an empty ring
        pp.any = false;
        int it = 0;
        for (int jj = shared_rho(r, s0, wq); jj < sh.my_nq; jj += wq, ++it) trace(it, group_of(jj, 0), shade_run);
        // the ring's last group.  (These three lines and their twin below the per-iteration loops stay written out: as a lambda or a
        // function template, alone or shared with trace(), they cost the exact build's two shared ring instances their seventh wave —
        // 74 VGPRs instead of 72, or 12 B / lane of scratch under the bound.)
        if constexpr (RING) {
          if (pp.any) {
            carry_drain_to<true, 2, kD0, true>(ws, pp.mark, lane, nodes, geoms);
            shade_run(ws.best[pp.par * 64 + lane], ws.rec + pp.par * 6 * 64 + lane, pp.g);
          }
        }
        // the run's counts, one lane per iteration (zeros where the wave had no chunk)
        if (lane < s1 - s0) rt.sub[(s0 + lane) * rt.wq0 + shared_rho(r, s0 + lane, wq)] = ((unsigned long long)(uint32_t)vnd << 32) | (uint32_t)vnl;
      }
    } else {
      int it = 0;
      for (int k = k0, rho = strand_rho(r, k0, wq); k < k1; ++k, rho = rho + 1 == wq ? 0 : rho + 1) {
        for (int jj = rho; jj < sh.my_nq; jj += wq, ++it) trace(it, group_of(jj, k), shade_group);
      }
      if constexpr (RING) {  // the ring's last group (see the shared form's tail)
        if (pp.any) {
          carry_drain_to<true, 2, kD0, true>(ws, pp.mark, lane, nodes, geoms);
          shade_group(ws.best[pp.par * 64 + lane], ws.rec + pp.par * 6 * 64 + lane, pp.g);
        }
      }
      if (!b.flat)
        while (ck < k1) next_iteration();  // the last iteration's counts, and zeros for trailing iterations without a chunk
    }
    if (plan.pieces == 1) break;
    int nx = 0;
    if (lane == 0) nx = atomicAdd(&qs.deal[deal_map(qs).strand_counter()], 1);
    strand = qs.W + __builtin_amdgcn_readfirstlane(nx);
  }
}

// ── ALL depths >= 1 in one launch: persistent lanes (k_paths) ─────────────────────────────────────────────────────────────────
// After depth 0 a path never goes back to HBM.  A wave has ONE set of 64 lanes; a lane carries its ray, its throughput, its
// sample id and ITS OWN depth.  When a path dies the lane writes the 16-byte retirement record and takes the next depth-1 ray
// of the wave's slice of its queue (k_primary's output); survivors stay where they are, at depth + 1.  The search, the
// candidate ring and the primitive-test chunks are per ray (candidates carry their owner lane), the RNG is keyed per lane by
// (iteration, pixel, depth), the retirement records by iteration: the results cannot differ from the per-depth kernels'.
// Traffic per PATH: its 40-byte depth-1 record read once, its 16-byte retirement record written once.
//   * per-LANE resolution: primitive tests only ever run as full 64-entry chunks, so a search leaves < 64 candidates in the
//     ring.  A lane is shaded as soon as the ring has processed the last candidate it filed (`mark`); the few lanes whose last
//     candidate is still pending sit out this round (~3 of 64 on cornell.txt) and are shaded in the next one, after the new
//     rays' candidates have pushed theirs through a full chunk.  (Rounds 1-3 kept two groups per wave for this and shaded a
//     group one iteration after its search: twice the lane state and LDS, four resident workgroups per CU instead of six.)
//   * refill: every lane owns a 40-byte LDS slot holding the NEXT path record it will take; the slot is filled by the
//     gfx950 LDS-direct loads (global_load_lds_dwordx4 / _dword: memory -> LDS without passing through VGPRs, LDS address =
//     M0 + lane * size), issued when the lane takes the previous one, i.e. at least a whole iteration before it is read.
//     The loads are inline assembly: the compiler's handling of the builtin either waits for the transfer at the very next
//     LDS access (it cannot tell the slot from the rest of the dynamic LDS) or does not compile under a divergent branch,
//     so the transfer, its s_waitcnt and the slot reads are all spelled out here.
//   * every vector-memory operation outstanding at the refill's s_waitcnt vmcnt(0) is a whole iteration old: the retirement
//     store of a lane that died is issued AFTER the slot reads of the next refill (the dead lane's colour and sample id
//     stay in its registers until then).
constexpr int kPathsWaves = 6;
constexpr int kPathsMinReady = 32;  // fewer resolved lanes than this and candidates pending: run the partial chunk instead of shading a thin group
PT_DEV uint32_t lds_offset(const void* p) { return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)p; }
// memory -> LDS without passing through VGPRs: path record i of a queue (b0 / b1 / b2 = the queue's first record in planes 0,
// 1, 2; wave-uniform, so they are scalar bases and a lane supplies 32-bit byte offsets only) of every active lane to lds_base
// (wave-uniform) + {0, 1024} + lane * 16 (planes 0 and 1) and + {2048, 2304} + lane * 4 (colour.z, sample id; pt_lds.h kSlotTail).  The
// instruction's immediate offset moves BOTH addresses, hence M0 + 0xfc for the last transfer.  M0 (the transfers' LDS base)
// belongs to the compiler: saved and restored.
template <typename T>
PT_DEV const T* uniform_ptr(const T* p) {  // a pointer the compiler cannot prove wave-uniform (derived from threadIdx.x >> 6), into scalar registers
  const uint64_t v = (uint64_t)(uintptr_t)p;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return reinterpret_cast<const T*>((uintptr_t)(((uint64_t)hi << 32) | lo));
}
PT_DEV void fetch_record_to_lds(const void* b0, const void* b1, const void* b2, int i, uint32_t lds_base) {
  uint32_t keep;
  const uint32_t off16 = (uint32_t)i << 4, off8 = (uint32_t)i << 3;
  asm volatile(
      "s_mov_b32 %[keep], m0\n\t"
      "s_mov_b32 m0, %[base]\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %[o16], %[b0]\n\t"
      "s_add_u32 m0, m0, 0x400\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %[o16], %[b1]\n\t"
      "s_add_u32 m0, m0, 0x400\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dword %[o8], %[b2]\n\t"
      "s_add_u32 m0, m0, 0xfc\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dword %[o8], %[b2] offset:4\n\t"
      "s_mov_b32 m0, %[keep]"
      : [keep] "=&s"(keep)
      : [base] "s"(lds_base), [b0] "s"(b0), [b1] "s"(b1), [b2] "s"(b2), [o16] "v"(off16), [o8] "v"(off8)
      : "memory", "scc");
}
// A split record (BatchInfo::split_records, pt_sched.h): the per-iteration word of path slot i from plane 0 and the invariant word
// of slot i0 from plane 1, to the same two 16-byte slot planes; the slot's 4-byte tail stays unused.
PT_DEV void fetch_split_to_lds(const void* b0, const void* b1, int i, int i0, uint32_t lds_base) {
  uint32_t keep;
  const uint32_t off = (uint32_t)i << 4, off0 = (uint32_t)i0 << 4;
  asm volatile(
      "s_mov_b32 %[keep], m0\n\t"
      "s_mov_b32 m0, %[base]\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %[o], %[b0]\n\t"
      "s_add_u32 m0, m0, 0x400\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %[o0], %[b1]\n\t"
      "s_mov_b32 m0, %[keep]"
      : [keep] "=&s"(keep)
      : [base] "s"(lds_base), [b0] "s"(b0), [b1] "s"(b1), [o] "v"(off), [o0] "v"(off0)
      : "memory", "scc");
}
// The whole record waiting in a lane's refill slot (fetch_record_to_lds) and its visit word, once every vector-memory operation has
// landed: everything outstanding here (last refill's transfers, last refill's retirement stores) is a whole iteration old.
PT_DEV void read_record_slot(uint32_t s16, uint32_t s4, v4f& w0, v4f& w1, float& cz, int& nslot, int& nrs) {
  asm volatile(
      "s_waitcnt vmcnt(0)\n\t"
      "ds_read_b128 %0, %5\n\t"
      "ds_read_b128 %1, %5 offset:1024\n\t"
      "ds_read_b32 %2, %6\n\t"
      "ds_read_b32 %3, %6 offset:256\n\t"
      "ds_read_b32 %4, %6 offset:512\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(w0), "=&v"(w1), "=&v"(cz), "=&v"(nslot), "=&v"(nrs)
      : "v"(s16), "v"(s4)
      : "memory");
}
// Per-wave LDS of k_paths: closest-hit keys, winner records, the candidate ring (16-bit entries: top entry << 6 | owner lane;
// the chunk looks leaf and geom index up in tword[top entry] = leaf | geom << 8, so it does not go through nodes[leaf]) and the
// running totals.  The rays are NOT kept in LDS: the lanes are persistent, a chunk fetches a candidate's ray from its owner's
// registers (ds_bpermute).
struct Lanes {
  unsigned long long* best;  // [64]
  float* rec;                // [6][64]  normal xyz, point xyz
  uint16_t* ent;             // [kRing]
  int head, count;           // wave-uniform
  int appended, processed;   // running totals (wave-uniform)
};
PT_DEV Lanes lanes_init(char* base) {  // on a LanesMap::bytes block
  Lanes c;
  c.best = reinterpret_cast<unsigned long long*>(base + LanesMap::best);
  c.rec = reinterpret_cast<float*>(base + LanesMap::rec);
  c.ent = reinterpret_cast<uint16_t*>(base + LanesMap::ent);
  c.head = c.count = c.appended = c.processed = 0;
  return c;
}
// Primitive tests for the first n (<= 64) pending entries; wave-uniform control flow, all 64 lanes active.
PT_DEV void paths_chunk(Lanes& c, int n, int lane, f3 o, f3 d, const uint32_t* tword, const ptd::Geom* __restrict__ geoms) {
  const bool valid = lane < n;
  const uint32_t entry = c.ent[(c.head + lane) & (kRing - 1)];
  const int src = (int)(entry & 63u);
  const uint32_t tw = tword[valid ? entry >> 6 : 0u];
  const uint32_t leaf = tw & 255u;
  const f3 ro = mk(bperm(src, o.x), bperm(src, o.y), bperm(src, o.z));
  const f3 rd = mk(bperm(src, d.x), bperm(src, d.y), bperm(src, d.z));
  const ptd::Geom* G = geoms + (valid ? (int)(tw >> 8) : 0);
  f3 pt = mk(0.f, 0.f, 0.f), nrm = mk(0.f, 0.f, 0.f);
  const float t = geom_test<-1, false>(G, ro, rd, pt, nrm, mk(0.f, 0.f, 0.f));
  // keep_closest and (k_paths' shading) resolve_hit written out: through them k_paths on cornell took 1149.9 us against 1144.5 (fast)
  const uint32_t tb = __float_as_uint(t);
  if (valid && t > 0.f && tb < 0x7f7fffffu) {
    const unsigned long long key = ((unsigned long long)tb << 32) | leaf;
    unsigned long long* slot = &c.best[src];
    atomicMin(slot, key);
    if (*slot == key) {  // this candidate is the ray's best so far: publish its record
      float* r = c.rec + src;
      r[0 * 64] = nrm.x, r[1 * 64] = nrm.y, r[2 * 64] = nrm.z;
      r[3 * 64] = pt.x, r[4 * 64] = pt.y, r[5 * 64] = pt.z;
    }
  }
  c.head = (c.head + n) & (kRing - 1);
  c.count -= n;
  c.processed += n;
}
// Candidate search of the fresh lanes of a persistent group (LDS-table scenes: every top entry is a leaf) — carry_search's
// two-phase form with the per-lane resolution mark: `mark` = ring entries appended up to and including the lane's last one.
// tword[e] = leaf | geom << 8 of top entry e (read by the chunks).
typedef __attribute__((address_space(4))) const v4f cfloat4;  // wave-uniform indices into it become scalar loads (a builtin vector: HIP's float4 class cannot be copied out of another address space)
template <typename TOP>
PT_DEV void paths_search(Lanes& c, TOP* top, const uint32_t* tword, int ntop, const ptd::Geom* __restrict__ geoms, f3 o, f3 d,
                         bool fresh, int lane, int& mark) {
  const RayInv ri = ray_inv(d, o);
  if (fresh) {
    c.best[lane] = kNoHit;
    mark = c.processed;  // no candidate: resolved at once
  }
  // box tests, eight at a time fully unrolled (no loop-carried box registers to rotate); bit (ntop - 1 - e) of the mask = entry e
  // (carry_search<SUB = false> restates this two-phase search; fetching four boxes together before testing them — one wait for four
  // scalar loads instead of one per box — was measured in the fast build: k_paths 1292 -> 1315 us, 32 more SGPRs in flight and 19 spilled)
  uint32_t mask = 0;
  for (int e0 = 0; e0 < ntop; e0 += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = e0 + u;
      if (e < ntop) {
        const auto A = top[2 * e], B = top[2 * e + 1];
        mask = push_bit(mask, slab(o, ri, A.x, A.y, A.z, A.w, B.x, B.y));
      }
    }
  }
  mask = fresh ? mask : 0u;
  while (true) {
    const unsigned long long m = ballot(mask != 0u);
    if (!m) break;
    const int rank = rank_in(m);
    if (mask != 0u) {
      const int te = ntop - 1 - __builtin_ctz(mask);
      mask &= mask - 1u;
      c.ent[(c.head + c.count + rank) & (kRing - 1)] = (uint16_t)((te << 6) | lane);
      if (mask == 0u) mark = c.appended + rank + 1;
    }
    const int cnt = __popcll(m);
    c.count += cnt;
    c.appended += cnt;
    if (c.count >= 64) paths_chunk(c, 64, lane, o, d, tword, geoms);
  }
}
// kLdsTables (mode 0): scene tables in LDS, every leaf a top entry (cornell.txt: the form described above).
// kTopScan (mode 1): tables in memory, top list + per-lane subtree scans with work stealing (carry_search<true>);
// kGrid (mode 2): tables in memory, uniform grid walk (grid_search).  Modes 1 and 2 run every pending candidate before they shade
//         (a search of theirs files several chunks' worth, and stolen work files candidates under other lanes' names, so a
//         per-lane mark would need cross-lane bookkeeping): all live lanes are searched and shaded in every round.
//         The grid walk's rings leave no LDS for refill slots (three workgroups per CU with them: measured 17-22 % slower than
//         the per-depth kernel it replaces), and its rounds take tens of microseconds: the next record of a lane waits in
//         REGISTERS there, loaded a round ahead by ordinary loads (waves per SIMD: see kPathsGridWaves; prefetching only origin
//         and direction and loading the rest on demand: slower).
// Waves per SIMD of modes 1 and 2 (mode 0: kPathsWaves).  Mode 2: 95-96 VGPRs without scratch since the wave index is scalar;
// in-box 4 and 5 are level for the fast build, 5 wins for exact.
constexpr int kPathsScanWaves = 5, kPathsGridWaves = 5;
// k_paths' visit ring (fillc): one record counter per sub-list visit of the cursor, kVisitRing per wave, taken modulo the ring.
// A refill starts only while every path in flight was taken fewer than kVisitLap visits ago; it makes at most kVisitsPerRefill
// new visits and the seek of a new piece one more, so no counter of a path in flight is handed to another visit.
constexpr int kVisitLap = 32, kVisitsPerRefill = 31;
static_assert(kVisitLap + kVisitsPerRefill + 1 <= kVisitRing, "the visit ring laps a path in flight");
static_assert((kVisitRing & (kVisitRing - 1)) == 0, "visit numbers wrap with a mask");
// SPLIT (BatchInfo::split_records, pt_sched.h): a path's record is the per-iteration word (direction, sample id | specular bit) at its
// own slot of plane 0 and the invariant word (origin, material index) at the same slot of ITERATION 0 in plane 1 — the cursor
// keeps both bases — and its throughput is (1, 1, 1) times the material's spec or color, formed when the lane takes the path.
// SPLIT == kFirstBounce (BatchInfo::split_records 2, MODE 0 only; pt_sched.h batch_form): the record is the pixel's one whole record at
// the slot of iteration 0; the iteration comes from the cursor and waits beside the visit number (pack_visit), and the lane that
// takes the record decides depth 0 and samples the first bounce itself, in the rotated loop behind the other forms'.
// SPLIT == kFixedSlots (such a batch with BatchInfo::fixed_slots; pt_sched.h batch_form): the first-bounce form without the visit ring — the
// cursor keeps where the record of its sub-list's first path goes, the word that waits beside a record is the path's own record slot
// (pack_fixed), and a dying lane has nothing to ask anybody: no counter, no lap guard, no limit on the visits of a refill.
// PREV (empty, or PrevGather alone; kFixedSlots only — pt_sched.h gather_plan): the launch also gathers the batch before its own, whose
// records lie in the other record plane.  The waves of queue q add that batch's records of queue q to the image, stream_gather_slot's
// work for 64 consecutive slots at a time: group j of the queue's my_nq goes to wave j mod wq, which takes one group each time it moves
// on to a piece (not the first: nothing is in flight beside it then) and the rest of its share after its last path has retired.  A step
// is synchronous — loads, wait, adds, stores — and stands where no transfer into the refill slots is younger than a round, so the
// refill's accounting of what is outstanding is what it was; its time is taken off the ticks the wave reports for the deal.
constexpr int kInlineGroup = 8;  // loads in flight per lane in a step
template <int GROUP>
PT_DEV void stream_gather_slot(int N, int K, const QueueShare& sh, const ptd::RetireBuf& ret, const ptd::Word4* plane, const ptd::Word4* front,
                               float* __restrict__ image, int q, int s);  // pt_output.inc
// Wave-uniform state that only the cold sites of k_paths<kLdsTables, ..> read — the piece switch, seek, a gather step, the epilogue — is
// not kept in scalar registers across the round: the kernel has more of it than the scalar file holds, and what does not fit is
// parked in the lanes of a VGPR and comes back through v_readlane_b32, a vector instruction, in whichever block the register allocator
// picks (tools/isa_spills.py).  Kernel arguments are read again where they are used, from the kernarg segment through the
// scalar cache (PathsArgs mirrors the segment: the arguments by value, in order, each at its natural alignment); a value computed in
// the prologue passes through cold(), behind which whatever is derived from it stays at the site instead of being hoisted to the
// loop's entry and parked.  Neither may stand where a round passes every time: a scalar load there is a wait per round.
template <typename... PREV>
struct PathsPrev {};
template <typename P>
struct PathsPrev<P> {
  P p;
};
template <typename... PREV>
struct PathsArgs {
  SceneTables sc;
  BatchInfo b;
  ptd::Queues qs;
  int32_t* cnt;
  ptd::PathBuf in;
  ptd::RetireBuf ret;
  PathsPrev<PREV...> prev;
};
template <typename A>
PT_DEV const A& cold_args() {
  auto p = __builtin_amdgcn_kernarg_segment_ptr();  // (constant address space: scalar loads)
  asm volatile("" : "+s"(p));  // (the loads behind it cannot be merged with the prologue's or moved above this point)
  return *(const A*)p;
}
PT_DEV int cold(int v) {
  asm volatile("" : "+s"(v));
  return v;
}
template <Search MODE, int SPLIT = 0, typename... PREV>
__global__ __launch_bounds__(kBlock, MODE == 0 ? kPathsWaves : MODE == 1 ? kPathsScanWaves : kPathsGridWaves) void k_paths(SceneTables sc, BatchInfo b, ptd::Queues qs, int32_t* __restrict__ cnt /* [depth][Q] rows */,
                                                               ptd::PathBuf in, ptd::RetireBuf ret, PREV... prev) {
  extern __shared__ float4 lds_raw[];
  char* lds = reinterpret_cast<char*>(lds_raw);
  const PathsLds L = paths_lds<MODE, kFast>(sc);
  stage16(lds + L.top, sc.top_b, MODE == 2 ? 0 : top_bytes(sc));  // the bounce kernels' box tables (SceneTables::*_b); the grid walk replaces top list and subtrees
  stage16(lds + L.mats, sc.mats, mat_bytes(sc));
  const float4* top = reinterpret_cast<const float4*>(lds + L.top);
  const ptd::Mat* mats = reinterpret_cast<const ptd::Mat*>(lds + L.mats);
  const ptd::Node* nodes = sc.nodes_b;
  const ptd::Geom* geoms = sc.geoms;
  if (MODE == 0) {  // the geometry records; of the nodes only tword / lmat below are needed (every leaf is a top entry)
    stage16(lds + L.geoms, sc.geoms, geom_bytes(sc));
    geoms = reinterpret_cast<const ptd::Geom*>(lds + L.geoms);
  }
  const char* lnodes = nullptr;
  if (MODE == 1 && sc.scan_nodes_lds > 0) {
    stage16(lds + L.nodes, sc.nodes_b, node_bytes(sc));
    lnodes = lds + L.nodes;
  }
  using WM = PathsWaveMap<MODE, kFast>;
  constexpr bool FIXED = SPLIT == kFixedSlots, FIRST = SPLIT == kFirstBounce || FIXED;  // FIRST: the first bounce is sampled here
  constexpr bool GATHER = sizeof...(PREV) > 0;
  static_assert(!GATHER || FIXED, "only a batch with fixed record slots gathers its predecessor");
  // COLD: the cold sites read the arguments from the kernarg segment (cold_args); the other search forms keep them as they were
  constexpr bool COLD = MODE == kLdsTables;
  using Args = PathsArgs<PREV...>;
  auto c_b = [&]() -> const BatchInfo& {
    if constexpr (COLD) return cold_args<Args>().b;
    else return b;
  };
  auto c_qs = [&]() -> const ptd::Queues& {
    if constexpr (COLD) return cold_args<Args>().qs;
    else return qs;
  };
  const int he = iter_hash_entries(sc);
  uint32_t* tword = reinterpret_cast<uint32_t*>(lds + L.tword);  // MODE 0: [kMaxTop] leaf | geom << 8 per top entry
  int* lmat = reinterpret_cast<int*>(lds + L.lmat);              // MODE 0: [64] material of the leaf at threaded node index i
  uint32_t* ihash = reinterpret_cast<uint32_t*>(lds + L.ihash);  // rows of the depths 1 .. trace_depth - 1
  for (int d = 1; d < b.trace_depth; ++d) iter_hash_fill(ihash + (d - 1) * he, sc, b, d);
  for (int e = threadIdx.x; MODE == 0 && e < sc.num_top; e += blockDim.x) {
    const int leaf = sc.top[e].idx, gi = sc.nodes[leaf].geom;
    tword[e] = (uint32_t)leaf | ((uint32_t)gi << 8);
    lmat[leaf & 63] = sc.geoms[gi].material;
  }
  __syncthreads();
  const int wib = threadIdx.x >> 6;
  char* wbase = lds + L.waves + wib * L.wave_bytes;
  Lanes cy = lanes_init(wbase);  // MODE 0; its keys and records are where the other modes' Carry has them
  GridRings gr = grid_rings_init<false>(wbase);  // MODES 1, 2 (the same bytes; mode 1 uses the Carry alone)
  Carry<false, 1>& cb = gr.cy;
  CellRing& cr = gr.cr;
  cb.lnodes = (const __attribute__((address_space(3))) v4f*)(lnodes ? lnodes : lds), cb.lds_nodes = lnodes != nullptr;
  constexpr bool SLOTS = MODE == 0;
  char* slots = wbase + WM::slots;  // SLOTS: [64] x 16 B, [64] x 16 B, [64] x 4 B, [64] x 4 B, [64] x 4 B
  int* died = reinterpret_cast<int*>(wbase + WM::died);    // [64]: paths of this wave retired AT depth d (statistics; PT_MAX_DEPTH = 64)
  [[maybe_unused]] int* fillc = reinterpret_cast<int*>(wbase + WM::fillc);  // [kVisitRing]: next record slot per sub-list visit (FIXED: unused)
  const int ntop = sc.num_top;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + wib);  // (the compiler cannot see that threadIdx.x >> 6 is wave-uniform)
  const int lane = lane_id();
  died[lane] = 0;
  const uint64_t t_begin = __builtin_amdgcn_s_memrealtime();  // (100 MHz, whatever the shader clock does)
  // Which queue the wave serves, as which of how many: W / Q waves per queue, or — once a batch has been measured — the
  // queue's share of the W waves by the time its waves took in the previous batch (ptd::Queues::deal).
  const DealMap dm = deal_map(qs);
  const WaveSlot even = wave_slot(wave, qs.Q, qs.W);
  int q = even.q, r = even.r, wq = even.wq;
  if (qs.deal != nullptr && qs.deal[dm.made_for()] == qs.W) {
    int at_or_before = 0;  // first[] is strictly increasing: the queues whose first wave is <= this wave
    for (int e0 = 0; e0 < qs.Q; e0 += 64) at_or_before += (int)__popcll(ballot(e0 + lane < qs.Q && qs.deal[dm.first(e0 + lane)] <= wave));
    q = at_or_before - 1;
    const int first = qs.deal[dm.first(q)];
    r = wave - first, wq = qs.deal[dm.first(q + 1)] - first;
  }
  const Retire rt = retire_of(ret, q);
  const int64_t qbase = (int64_t)q * qs.cap;
  // The queue's depth-1 rays: k_primary's sub-lists (k, rho), e = k * wq0 + rho, concatenated in that order (their survivor
  // counts — the low words of sub[e] — are final before this launch).  A wave takes pieces [p * ps, (p + 1) * ps) of the global
  // ranks and walks each front to back with a cursor: the sub-list the next rank lies in, where that sub-list starts in the queue's
  // path region, and where the records of its paths go — the slots from retirees(e) + i on in sub-region e for the paths from
  // index i on (RetireBuf).
  const int wq0 = rt.wq0, ne = b.K * wq0;
  const QueueShare qshare = queue_share(b, qs, q);
  const int my_nq = qshare.my_nq, quo = my_nq / wq0, rem = my_nq % wq0;
  auto count_of = [&](int e) { return e < ne ? (int)(uint32_t)rt.sub[e] : 0; };
  // Every wave of the queue scans sub[] for the total and for where its slice begins.  With a small tile that is thousands of
  // words (an eighth of 1080p: 195 iterations x 20 residues): the words are fetched four 64-entry chunks ahead of their
  // reductions, and the chunk sums stay in a register (lane i: chunk i) so that the second scan starts at the slice's chunk.
  int total = 0, csum = 0;
  const bool chunk_sums = ne <= 64 * 64;
  for (int e0 = 0; e0 < ne; e0 += 256) {
    int n4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) n4[j] = count_of(e0 + 64 * j + lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int sum;
      (void)wave_prefix6(n4[j], sum);
      total += sum;
      if (lane == (e0 >> 6) + j) csum = sum;
    }
  }
  if (r == 0 && lane == 0) cnt[cnt_index(qs, 1, q)] = total;  // statistics: rays traced at depth 1
  // ... and at depth 0, k_primary's own figure: a first-bounce batch may run without that kernel (pt_sched.h batch_form), and the row is zeroed after every batch
  if constexpr (SPLIT == kFirstBounce || SPLIT == kFixedSlots)
    if (r == 0 && lane == 0) cnt[cnt_index(qs, 0, q)] = b.K * qshare.my_pixels;
  // The queue's ranks [0, total) are cut into pieces of `ps` paths.  Piece r is the wave's own; the pieces from wq on go, in
  // order, to whichever wave of the queue has finished what it had (a counter per queue behind ptd::Queues::deal, zeroed by
  // k_count_stats): equal numbers of depth-1 rays are not equal work — a piece's paths come from a few dozen pixel chunks, and
  // how long a path lives depends on where it starts (a wave of the equal-slices form was resident for 74 % of the launch on
  // average: SQ_WAVE_CYCLES against SQ_BUSY_CYCLES).  A wave streams its pieces through ONE set of lanes: it moves on to the
  // next piece while the last paths of the previous one are still in flight.  Which wave traces a path changes no sample.
  // Piece sizes fall: the pieces of level l = p / wq hold ps0 (1 - 1 / P)^l paths (not fewer than a refill's worth; tests: fewer),
  // ps0 = total / (wq P), P = paths_pieces, so that the levels add up to the queue — large pieces while everybody is busy, small
  // ones at the end, where a launch waits for the last piece (pieces of one size left half a piece of idle time per wave).
  const PiecePlan pieces0 = piece_plan(total, wq, b.paths_pieces, qs.deal != nullptr, chunk_sums);
  auto piece_plan_here = [&]() {  // (COLD: formed again at the switch from the total and the arguments — five registers less across the round)
    if constexpr (COLD) return piece_plan(cold(total), wq, c_b().paths_pieces, c_qs().deal != nullptr, cold(ne) <= 64 * 64);
    else return pieces0;
  };
  [[maybe_unused]] int clist0 = 0;  // SPLIT: clist without its iteration's k * seg_cap — where the sub-list of iteration 0 starts
  int ce = ne, cstart = total, ccnt = 0, clist = 0;  // cursor (wave-uniform): sub-list e = k * wq0 + rho; nothing to stream leaves it at the end
  int cord = 0;  // sub-list visits of the cursor so far
  // kFirstBounce: the cursor's iteration and its depth-0 hash iter_hash(iter_first + k, 0), formed where the cursor moves; next_h (per lane):
  // that hash of the record waiting in the lane's slot.  (Hashed per lane at the take instead: k_paths 12-20 us slower, profiles/first_bounce.log.)
  [[maybe_unused]] int cur_k = 0;
  [[maybe_unused]] uint32_t cur_h = 0u, next_h = 0u;
  // FIXED: the record slot of the cursor's sub-list's first path, without its iteration's k * seg_cap, and the bits it is packed in
  [[maybe_unused]] int crec0 = 0;
  [[maybe_unused]] const int fbits = fixed_bits(rt.seg_cap);
  // A window of 64 consecutive sub[] words in registers (lane l holds sub[win0 + l]): the cursor reads counts and retiree numbers
  // with v_readlane instead of a dependent global load per sub-list.  With a whole 1080p frame a wave's piece touches a handful of
  // sub-lists of ~1000 paths; with an eighth of it (eight GPUs, ~190 iterations per batch) dozens of sub-lists of ~25, a fifth of
  // them empty, and two memory round trips per sub-list were a fifth of the kernel's time.
  int win0 = -64;  // nothing loaded yet: no index e >= 0 lies in [-64, 0)
  unsigned long long wsub = 0ull;
  auto window_to = [&](int e) {  // make sub[e] available (wave-uniform e)
    if (e < win0 || e >= win0 + 64) {
      win0 = e;
      wsub = (e + lane < ne) ? rt.sub[e + lane] : 0ull;
    }
  };
  auto sub_word = [&](int e) -> unsigned long long {  // sub[e] for a wave-uniform e inside the window
    const uint32_t lo32 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)wsub, e - win0);
    const uint32_t hi32 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(wsub >> 32), e - win0);
    return ((unsigned long long)hi32 << 32) | lo32;
  };
  window_to(0);
  // The records of the paths a wave takes out of ONE visit of a sub-list fill a contiguous range of its sub-region, whatever
  // order they arrive in, so the wave appends them in order of retirement through a counter per visit in LDS (fillc, the visit
  // ring: lanes of one sub-list that die together get consecutive slots, as the per-iteration counters of the earlier layouts
  // gave).  A lane remembers the visit number of its path; the refill below keeps the ring from lapping a path in flight.
  auto cursor_bases = [&](int first_rank) {
    const int ec = min(ce, ne - 1), ck = ec / wq0, crho = ec - ck * wq0;  // (wave-uniform: scalar instructions)
    clist = ck * rt.seg_cap + sub_offset(quo, rem, crho) * 64;
    if constexpr (SPLIT != 0) clist0 = invariant_slot(clist, ck, rt.seg_cap);
    if constexpr (FIRST) cur_k = ck, cur_h = iter_hash(b.iter_first + ck, 0);  // (wave-uniform: the hash runs on the scalar unit)
    window_to(ec);
    const int crec = clist + (int)(uint32_t)(sub_word(ec) >> 32);
    if constexpr (FIXED) crec0 = invariant_slot(crec, ck, rt.seg_cap);  // (pt_sched.h fixed_slot: + the path's list position)
    else if (lane == 0) fillc[cord & (kVisitRing - 1)] = crec + (first_rank - cstart);  // where this wave's first record of the visit goes
  };
  // put the cursor on the sub-list that rank `at_rank` (< total) lies in: a new visit
  auto seek = [&](int at_rank) {
    int cum = 0, e_begin = 0;
    if (COLD ? cold(ne) <= 64 * 64 : chunk_sums) {
      int all;
      const int cbefore = wave_prefix6(csum, all);
      const unsigned long long here = ballot(csum > 0 && cbefore <= at_rank && at_rank < cbefore + csum);
      if (here) {
        const int l = __builtin_ctzll(here);
        e_begin = l * 64, cum = __builtin_amdgcn_readlane(cbefore, l);
      }
    }
    for (int e0 = e_begin; e0 < ne; e0 += 64) {
      const int n = count_of(e0 + lane);
      int sum;
      const int before = wave_prefix6(n, sum);
      const unsigned long long here = ballot(n > 0 && cum + before <= at_rank && at_rank < cum + before + n);
      if (here) {
        const int l = __builtin_ctzll(here);
        ce = e0 + l, cstart = cum + __builtin_amdgcn_readlane(before, l), ccnt = __builtin_amdgcn_readlane(n, l);
        break;
      }
      cum += sum;
    }
    ++cord;
    cursor_bases(at_rank);
  };
  // Path index (inside the queue's region) of the rays of global rank `rank`, for the lanes that `want` one (consecutive ranks in
  // lane order), and the visit their retirement records are counted under.  Ranks only grow inside a piece, so the cursor only
  // moves forward; it stops after kVisitsPerRefill new visits (sub-lists of a path or two: tiles of a few pixels per wave) — the lanes behind
  // that are served by a later refill.  Returns whether the lane was served.  Wave-uniform control flow.  (at0, SPLIT: the same index in iteration 0)
  auto assign = [&](bool want, int rank, int& at, [[maybe_unused]] int& at0, int& rs) -> bool {
    bool pending = want;
    const int cord0 = cord;
    while (true) {
      const bool in = pending && rank < cstart + ccnt;
      if (in) at = clist + (rank - cstart), rs = cord;
      if constexpr (SPLIT != 0)
        if (in) at0 = clist0 + (rank - cstart);
      if constexpr (FIRST)
        if (in) rs = (int)(FIXED ? pack_fixed(cur_k, crec0 + (rank - cstart), fbits) : pack_visit(cur_k, cord)), next_h = cur_h;  // the iteration waits with the record, its depth-0 hash in a register of the lane
      pending = pending && !in;
      if (!ballot(pending) || ce >= ne || (!FIXED && cord - cord0 >= kVisitsPerRefill)) break;
      cstart += ccnt;  // on to the next sub-list that holds anything: the first non-empty one behind ce in the window, else the window moves on
      ccnt = 0;
      int nxt = ce + 1;
      while (nxt < ne) {
        window_to(nxt);
        const unsigned long long holds = ballot((uint32_t)wsub != 0u) & (~0ull << (nxt - win0));
        if (holds) {
          nxt = win0 + (int)__builtin_ctzll(holds);
          ccnt = (int)(uint32_t)sub_word(nxt);
          break;
        }
        nxt = win0 + 64;
      }
      ce = min(nxt, ne);
      ++cord;
      cursor_bases(cstart);
    }
    return want && !pending;
  };
  const uint32_t s_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_offset(slots));
  const uint32_t s16 = s_base + (uint32_t)lane * 16u, s4 = s_base + (uint32_t)kSlotTail + (uint32_t)lane * 4u;
  // issue the transfer of path record `i` of the queue into this lane's slot
  const ptd::Word4 *in0 = uniform_ptr(in.r + qbase), *in1 = uniform_ptr(in.r + in.stride + qbase);
  const float* in2 = uniform_ptr(reinterpret_cast<const float*>(in.r + 2 * in.stride) + 2 * qbase);
  PathRec nx;  // !SLOTS: the lane's next record, in registers
  nx.o = nx.d = nx.c = mk(0.f, 0.f, 0.f), nx.tag = PathTag{0, 0u, 0};
  int nx_rs = 0;  // !SLOTS: ... and its visit
  int* slot_rs = reinterpret_cast<int*>(slots + kSlotVisit) + lane;  // SLOTS: the visit of the record waiting in the lane's slot
  auto fetch = [&](int at, [[maybe_unused]] int at0, int rs) {
    if constexpr (SLOTS && SPLIT == kSplitRecords) fetch_split_to_lds(in0, in1, at, at0, s_base), *slot_rs = rs;
    else if constexpr (SLOTS) fetch_record_to_lds(in0, in1, in2, FIRST ? at0 : at, s_base), *slot_rs = rs;  // (first bounce: the pixel's one record)
    else if constexpr (SPLIT == kSplitRecords) {  // the two words as they lie in memory: unpacked when the lane takes them
      const ptd::Word4 w0 = in.r[qbase + at], w1 = in.r[in.stride + qbase + at0];
      nx.o = mk(w0.x, w0.y, w0.z), nx.d = mk(w0.w, w1.x, w1.y), nx.c = mk(w1.z, w1.w, 0.f), nx_rs = rs;
    } else nx = path_load(in, qbase + at), nx_rs = rs;
  };
  // Tile pixel -> global pixel at the take.  The form is fixed for the launch: a contiguous tile costs one add from one register.  The
  // striped and the list form fetch their five fields at the head of the refill (refill_pixel_map: independent scalar loads from one
  // pointer, issued in front of the slot's LDS reads, so they land under the wait the refill has anyway) and keep nothing across the round.
  const int pix0 = b.stripe == 0 && b.pixel_begin >= 0 ? b.pixel_begin : -1;
  auto refill_pixel_map = [&]() {
    PixelMap pm{0, 0, 0, 0.f, nullptr};
    if constexpr (COLD)
      if (pix0 < 0) pm = pixel_map(c_b());
    return pm;
  };
  auto pixel_of = [&](const PixelMap& pm, int pl) {
    if constexpr (COLD) {
      if (pix0 >= 0) return pix0 + pl;
      return global_pixel(pm, pl);
    } else return global_pixel(b, pl);
  };
  // fast build: the top list's base for the search's scalar loads, a value of its own — left an argument, the compiler may read it from the
  // kernarg segment again in every round (a scalar load and its wait at the top of the search) instead of keeping it
  [[maybe_unused]] uintptr_t top_b_scalar = (uintptr_t)sc.top_b;
  if constexpr (COLD && kFast) asm volatile("" : "+s"(top_b_scalar));
  // lane state
  f3 o = mk(0.f, 0.f, 0.f), d = o, c = o;
  int slot = 0, depth = 1, mark = 0, rslot = 0;  // rslot: the visit the path was taken in; from its death on: its record slot
  uint32_t phash = 0u;
  bool valid = false, fresh = false, owes = false;  // owes: the lane's path died and its retirement record is not stored yet
  bool has_next = false;                            // a record is waiting in the lane's slot (on its way there)
  int streamed = 0, p_hi = 0;  // the current piece: records [.., streamed) handed out, the piece ends at p_hi; -1: no piece left for this wave
  // GATHER: the wave's next group of the previous batch's slots, and the time its steps took (100 MHz ticks)
  [[maybe_unused]] int gj = r;
  [[maybe_unused]] uint32_t gather_time = 0u;
  [[maybe_unused]] auto gather_step = [&]() {
    if constexpr (GATHER) {
      const Args& ka = cold_args<Args>();  // (everything a step needs but the wave's place in it: nothing of it is kept across the round)
      const PrevGather& pg = ka.prev.p;
      const int gq = cold(q);
      const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
      stream_gather_slot<kInlineGroup>(ka.b.N, pg.K, queue_share(ka.b, ka.qs, gq), ka.ret, pg.rec, pg.plane0, pg.image, gq, gj * 64 + lane);
      gj += wq;
      gather_time += (uint32_t)(__builtin_amdgcn_s_memrealtime() - t0);
    }
  };
  while (!FIRST) {  // (that form's loop, the same round rotated, follows this one)
    // ── on to the wave's next piece, once the current one is handed out: its own, then whatever the queue's counter gives ──
    if (streamed >= p_hi && p_hi >= 0) {
      const PiecePlan pieces = piece_plan_here();
      int nextp = -1;
      if (cord == 0) nextp = r;  // (every piece starts with a visit)
      else if (pieces.needs_counter()) {
        int v = 0;
        if (lane == 0) v = atomicAdd(&c_qs().deal[deal_map(c_qs()).piece_counter(q)], 1);
        nextp = wq + __builtin_amdgcn_readfirstlane(v);
      }
      const PieceRange pr = pieces.piece_range(nextp);
      if (pr.some) {
        streamed = pr.start, p_hi = pr.end;
        seek(streamed);
      } else {
        p_hi = -1;
      }
    }
    // ── refill: dead lanes take the record waiting in their slot; the slot gets the next record of the piece ──
    const bool take = !valid && has_next;
    if (ballot(take || owes || (!valid && !has_next && streamed < p_hi))) {
      const PixelMap pm = refill_pixel_map();
      v4f w0, w1;
      float cz;
      int nslot, nrs;
      if constexpr (SLOTS && SPLIT == kSplitRecords) {
        asm volatile(
            "s_waitcnt vmcnt(0)\n\t"
            "ds_read_b128 %0, %3\n\t"
            "ds_read_b128 %1, %3 offset:1024\n\t"
            "ds_read_b32 %2, %4 offset:512\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(w0), "=&v"(w1), "=&v"(nrs)
            : "v"(s16), "v"(s4)
            : "memory");
        cz = 0.f, nslot = 0;
      } else if constexpr (SLOTS) {
        read_record_slot(s16, s4, w0, w1, cz, nslot, nrs);
      } else {
        w0 = v4f{nx.o.x, nx.o.y, nx.o.z, nx.d.x}, w1 = v4f{nx.d.y, nx.d.z, nx.c.x, nx.c.y}, cz = nx.c.z, nslot = nx.tag.slot, nrs = nx_rs;
      }
      if (owes) {  // the record of the path that died in this lane (its colour and sample id are still here)
        rt.rec[rslot] = ptd::Word4{c.x, c.y, c.z, __int_as_float(slot & ((1 << b.slot_shift) - 1))};
        owes = false;
      }
      if constexpr (SPLIT == kSplitRecords) {  // (per-iteration word, invariant word)
        if (take) {
          const uint32_t word = __float_as_uint(w0.w);
          const ptd::Mat* m = mats + __float_as_int(w1.w);
          nslot = kind_sample_id(word);
          o = mk(w1.x, w1.y, w1.z), d = mk(w0.x, w0.y, w0.z);
          c = mul(mk(1.0f, 1.0f, 1.0f), kind_specular(word) ? mk(m->spec[0], m->spec[1], m->spec[2]) : mk(m->color[0], m->color[1], m->color[2]));
        }
      } else if (take) o = mk(w0.x, w0.y, w0.z), d = mk(w0.w, w1.x, w1.y), c = mk(w1.z, w1.w, cz);
      if (take) {
        slot = nslot, rslot = nrs;
        phash = utilhash((uint32_t)pixel_of(pm, nslot & ((1 << b.slot_shift) - 1)));
        depth = 1;
        valid = fresh = true;
        has_next = false;
      }
      // every lane without a waiting record gets the next one of the piece — unless a path in flight was taken kVisitLap or more visits
      // ago: its counter in the visit ring must not be handed to another visit (the cursor moves by at most kVisitsPerRefill per refill)
      const bool lapping = ballot(valid && cord - rslot >= kVisitLap) != 0ull;
      const bool empty = !has_next && !lapping;  // takers (just emptied) and lanes that found nothing at an earlier refill
      const unsigned long long em = ballot(empty);
      const int rank = rank_in(em);
      const bool more = empty && streamed + rank < p_hi;
      int at = 0, at0 = 0, rs = 0;
      const bool served = assign(more, streamed + rank, at, at0, rs);
      if (served) {
        has_next = true;
        fetch(at, at0, rs);
      }
      streamed += (int)__popcll(ballot(served));
    }
    // (no valid lane but records on their way, at the start of the wave: the rest of the round finds nothing to do — a `continue`
    // here costs six VGPRs)
    if (!ballot(valid || has_next) && p_hi < 0) break;  // every path of the wave's pieces has retired
    bool ready;
    if constexpr (MODE == 0) {
      // ── search: box tests + appends for the lanes with a new ray; full chunks as the ring fills ──
      if (ballot(fresh)) {
        // fast build: the top list's boxes come through scalar loads (constant address space: s_load into SGPRs, the scalar cache)
        // instead of broadcast LDS reads into VGPRs: 73 -> 67 VGPRs; in-box fast +0.8 %, exact -1.4 % (its longer tests cover the LDS latency)
        if constexpr (kFast) paths_search(cy, (cfloat4*)top_b_scalar, tword, ntop, geoms, o, d, fresh, lane, mark);
        else paths_search(cy, top, tword, ntop, geoms, o, d, fresh, lane, mark);
      }
      // ── which lanes are resolved?  Too few, with candidates pending: run them as a partial chunk ──
      ready = valid && (cy.processed - mark) >= 0;
      if (cy.count > 0 && __popcll(ballot(ready)) < kPathsMinReady) {
        paths_chunk(cy, cy.count, lane, o, d, tword, geoms);  // count < 64 here
        ready = valid;
      }
    } else {
      // ── search of every live lane (all of them have a new ray), then all its candidates ──
      cb.best[lane] = kNoHit;
      if constexpr (MODE == 2) grid_search<1>(cb, cr, sc, nodes, geoms, o, d, valid, lane, 0);
      else {
        PT_STAT(14, 1);
        PT_STAT(15, __popcll(ballot(valid)));
        carry_search<true, 1>(cb, top, ntop, nodes, geoms, o, d, valid, lane, 0, sc.cull_margin, sc.top_xor);
      }
      while (cb.count > 0) carry_chunk<false, 1, false, MODE == 2>(cb, min(64, cb.count), lane, nodes, geoms);
      ready = valid;
    }
    fresh = false;
    // ── shade the resolved lanes ──
    {
      ShadeIO s;
      s.o = mk(0.f, 0.f, 0.f);
      s.d = d;
      s.c = c;
      s.alive = false;
      Bounce bo;
      bo.kind = 0;
      const int k = (int)((uint32_t)slot >> b.slot_shift);
      const unsigned long long best = cy.best[lane];
      Hit h{false, -1.0f, -1, 0, mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 0.f)};  // resolve_hit's unpacking written out (see paths_chunk)
      if (ready) {
        if ((uint32_t)(best >> 32) != 0x7f7fffffu) {
          h.t = __uint_as_float((uint32_t)(best >> 32));
          const float* rr = cy.rec + lane;
          h.n = mk(rr[0 * 64], rr[1 * 64], rr[2 * 64]);
          h.p = mk(rr[3 * 64], rr[4 * 64], rr[5 * 64]);
          if constexpr (MODE == 0) {
            h.mat = lmat[(uint32_t)best & 63u];
          } else {
            const ptd::Geom* G = geoms + nodes[(uint32_t)best].geom;
            h.mat = G->material;
            if (MODE == 2) h.n = finish_normal(G, h.n);  // the grid's chunks leave the normal to the winner (carry_chunk, LEAN)
          }
        }
        const uint32_t ih = he > 0 ? ihash[(depth - 1) * he + k] : iter_hash(b.iter_first + k, depth);
        bo = shade_decide(mats, b.trace_depth, depth, ih ^ phash, h.t, h.mat, s);
      }
      const bool alive = ready && s.alive, dead = ready && !s.alive;
      if (dead) atomicAdd(&died[depth & 63], 1);  // statistics: rays traced at depth d = paths retired at depth >= d
      if (dead) rslot = atomicAdd(&fillc[rslot & (kVisitRing - 1)], 1);  // lanes of one visit get consecutive record slots
      if (alive) shade_bounce(bo, h.n, h.p, s);
      if (ready) {
        c = s.c;
        if (alive) o = s.o, d = s.d, depth += 1, fresh = true;
        else valid = false, owes = true;
      }
    }
  }
  // ── BatchInfo::split_records 2 (pt_sched.h batch_form): the same round, rotated ────────────────────────────────────────────
  // search, shade_decide of the resolved lanes, pieces + refill, direction sampling.  The refill above follows the shading at once
  // anyway; here it sits between shade_bounce's two halves, so a lane whose path has just died — or that never had one — takes its
  // next record, decides depth 0 for it (shade_decide's own depth-0 path: the seed of the record's iteration, at most one draw, the
  // throughput (1, 1, 1) times spec or color) and samples the path's first bounce in the instruction stream that samples the
  // survivors' next one, in lanes that would sit it out.  Across the refill a lane holds the new origin, the axis and the Bounce instead
  // of hit point, normal and old direction.  A taken path leaves the round at depth 1, fresh: it never sees a search at depth 0.
  // Memory ordering as above: a slot is read a round or more after its transfer was issued, the retirement store of a path that died
  // in this round's decide is issued after the slot reads, and what is outstanding at the wait is a whole round old.  Start
  // (nothing to search or decide, the refill fetches) and end (nothing valid, waiting or left after a refill) are ordinary rounds.
  if constexpr (FIRST) {
    static_assert(MODE == kLdsTables, "the first-bounce form takes its records from the refill slots of the LDS-table form");
    while (true) {
      // ── search: box tests + appends for the lanes with a new ray; too few resolved lanes with candidates pending: a partial chunk ──
      if (ballot(fresh)) {
        if constexpr (kFast) paths_search(cy, (cfloat4*)top_b_scalar, tword, ntop, geoms, o, d, fresh, lane, mark);
        else paths_search(cy, top, tword, ntop, geoms, o, d, fresh, lane, mark);
      }
      bool ready = valid && (cy.processed - mark) >= 0;
      if (cy.count > 0 && __popcll(ballot(ready)) < kPathsMinReady) {
        paths_chunk(cy, cy.count, lane, o, d, tword, geoms);  // count < 64 here
        ready = valid;
      }
      fresh = false;
      // ── decide for the resolved lanes; a survivor's new origin and axis ──
      Bounce bo;
      bo.kind = 0, bo.rng_x = 1u, bo.roughness = 0.f;
      f3 axis = mk(0.f, 0.f, 0.f);
      bool go = false;  // the lane samples a direction in this round
      {
        ShadeIO s;
        s.o = mk(0.f, 0.f, 0.f);
        s.d = d;
        s.c = c;
        s.alive = false;
        const int k = (int)((uint32_t)slot >> b.slot_shift);
        const unsigned long long best = cy.best[lane];
        Hit h{false, -1.0f, -1, 0, mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 0.f)};
        if (ready) {
          if ((uint32_t)(best >> 32) != 0x7f7fffffu) {
            h.t = __uint_as_float((uint32_t)(best >> 32));
            const float* rr = cy.rec + lane;
            h.n = mk(rr[0 * 64], rr[1 * 64], rr[2 * 64]);
            h.p = mk(rr[3 * 64], rr[4 * 64], rr[5 * 64]);
            h.mat = lmat[(uint32_t)best & 63u];
          }
          const uint32_t ih = he > 0 ? ihash[(depth - 1) * he + k] : iter_hash(b.iter_first + k, depth);
          bo = shade_decide(mats, b.trace_depth, depth, ih ^ phash, h.t, h.mat, s);
        }
        const bool alive = ready && s.alive, dead = ready && !s.alive;
        if (dead) atomicAdd(&died[depth & 63], 1);
        if constexpr (!FIXED)
          if (dead) rslot = atomicAdd(&fillc[rslot & (kVisitRing - 1)], 1);
        if (ready) {
          c = s.c;
          if (alive) {
            const BounceAxis a = bounce_axis(bo, h.n, h.p, d);
            o = a.o, axis = a.f, go = true;
          } else valid = false, owes = true;
        }
      }
      // ── on to the wave's next piece, once the current one is handed out ──
      if (__builtin_expect(streamed >= p_hi && p_hi >= 0, 0)) {  // (rare: the register allocator parks what only this block reads, not the round's state)
        if constexpr (GATHER)
          if (cord != 0 && gj < my_nq) gather_step();
        const PiecePlan pieces = piece_plan_here();
        int nextp = -1;
        if (cord == 0) nextp = r;
        else if (pieces.needs_counter()) {
          int v = 0;
          if (lane == 0) v = atomicAdd(&c_qs().deal[deal_map(c_qs()).piece_counter(q)], 1);
          nextp = wq + __builtin_amdgcn_readfirstlane(v);
        }
        const PieceRange pr = pieces.piece_range(nextp);
        if (pr.some) {
          streamed = pr.start, p_hi = pr.end;
          seek(streamed);
        } else {
          p_hi = -1;
        }
      }
      // ── refill: lanes without a path take the record waiting in their slot and decide its depth 0; the slot gets the next record ──
      const bool take = !valid && has_next;
      if (ballot(take || owes || (!valid && !has_next && streamed < p_hi))) {
        const PixelMap pm = refill_pixel_map();
        v4f w0, w1;
        float cz;
        int word, vword;
        read_record_slot(s16, s4, w0, w1, cz, word, vword);
        if (owes) {
          rt.rec[rslot] = ptd::Word4{c.x, c.y, c.z, __int_as_float(slot & ((1 << b.slot_shift) - 1))};
          owes = false;
        }
        if (take) {  // (bounce origin, hit normal, camera direction, pixel | material) and iteration | visit
          const int pl = first_pixel(word, b.slot_shift), k = FIXED ? fixed_k((uint32_t)vword, fbits) : visit_k((uint32_t)vword);
          const f3 hn = mk(w0.w, w1.x, w1.y), cam_d = mk(w1.z, w1.w, cz);
          slot = make_slot(b, k, pl), rslot = FIXED ? fixed_slot_of((uint32_t)vword, fbits, rt.seg_cap) : visit_number((uint32_t)vword);  // (FIXED: the record slot at once)
          phash = utilhash((uint32_t)pixel_of(pm, pl));
          ShadeIO s;
          s.o = mk(0.f, 0.f, 0.f);
          s.d = cam_d;
          s.c = mk(1.0f, 1.0f, 1.0f);
          s.alive = false;
          bo = shade_decide(mats, b.trace_depth, 0, next_h ^ phash, 0.0f, first_material(word, b.slot_shift), s);  // a hit, and no emitter's: it survives
          o = mk(w0.x, w0.y, w0.z), c = s.c;
          axis = bo.kind == 1 ? bounce_reflect(cam_d, hn) : hn;
          depth = 0;
          valid = go = true;
          has_next = false;
        }
        // (rslot of a path in flight: its visit modulo the packed width, as it waited in the slot)
        bool lapping = false;  // (FIXED: no ring to lap)
        if constexpr (!FIXED) lapping = ballot(valid && visit_gap(cord, rslot) >= kVisitLap) != 0ull;
        const bool empty = !has_next && !lapping;
        const unsigned long long em = ballot(empty);
        const int rank = rank_in(em);
        const bool more = empty && streamed + rank < p_hi;
        int at = 0, at0 = 0, rs = 0;
        const bool served = assign(more, streamed + rank, at, at0, rs);
        if (served) {
          has_next = true;
          fetch(at, at0, rs);
        }
        streamed += (int)__popcll(ballot(served));
      }
      if (!ballot(valid || has_next) && p_hi < 0) break;  // every path of the wave's pieces has retired
      // ── direction sampling: this round's survivors and the lanes that took a path ──
      if (go) d = bounce_sample(bo, axis), depth += 1, fresh = true;
    }
  }
  if constexpr (GATHER) {
    while (gj < my_nq) gather_step();  // the rest of the wave's share
    if (r == 0)  // the records are consumed: zero counters for the next batch (k_collect_stream's block 0 of the queue)
      for (int i = lane, kmax = cold_args<Args>().ret.kmax; i < kmax; i += 64) cold_args<Args>().ret.cnt[(int64_t)q * kmax + i] = 0ull;
  }
  // statistics: rays traced at depth d >= 2 = this wave's paths retired at depth >= d (row 1 holds the queue's input count already)
  if (lane == 0) {
    int reached = 0, rays = 0;
    int32_t* const ecnt = COLD ? cold_args<Args>().cnt : cnt;
    for (int dd = min(c_b().trace_depth - 1, 63); dd >= 2; --dd) {
      reached += died[dd];
      rays += reached;
      if (reached) atomicAdd(&ecnt[cnt_index(c_qs(), dd, q)], reached);
    }
    // What this queue's paths cost, for the next batch's deal: the TIME its waves spent on them (the waves of a queue finish together
    // — they share its pieces — so the sum is waves x the queue's finishing time, and dealing in proportion to it moves the
    // finishing times together whatever a ray costs where).  Rays traced were the first measure: an eighth of 1080p kept waves
    // resident for 73 % of the launch with it.
    rays += reached + died[1];  // (the wave's rays: every path it took has retired somewhere)
    uint64_t spent = __builtin_amdgcn_s_memrealtime() - t_begin;
    if constexpr (GATHER) spent -= min(spent, (uint64_t)gather_time);  // (the previous batch's gather is not this queue's paths)
    const int ticks = (int)min(spent >> 6, (uint64_t)0x3ffff);  // units of 0.64 us; a queue's sum stays below 2^31
    const ptd::Queues& eq = c_qs();
    if (eq.deal != nullptr && rays) atomicAdd(&eq.deal[deal_map(eq).time(q)], ticks), atomicAdd(&eq.deal[deal_map(eq).rays(q)], rays);
  }
}

// PathsArgs against the kernel: the members' types in order ARE the parameter list, so an argument added, dropped or moved stops the build
// here instead of shifting what the cold sites read.  (A struct's members and a kernel's by-value arguments are both laid out in order, each
// at its natural alignment: equal lists give equal offsets.)
template <typename... PREV>
using PathsSignature = void (*)(decltype(PathsArgs<PREV...>::sc), decltype(PathsArgs<PREV...>::b), decltype(PathsArgs<PREV...>::qs), decltype(PathsArgs<PREV...>::cnt),
                                decltype(PathsArgs<PREV...>::in), decltype(PathsArgs<PREV...>::ret), PREV...);
static_assert(std::is_same<decltype(&k_paths<kLdsTables, kFixedSlots>), PathsSignature<>>::value, "PathsArgs does not mirror k_paths' arguments");
static_assert(std::is_same<decltype(&k_paths<kLdsTables, kFixedSlots, PrevGather>), PathsSignature<PrevGather>>::value, "PathsArgs does not mirror k_paths' arguments");
static_assert(std::is_same<decltype(PathsArgs<PrevGather>::prev.p), PrevGather>::value && std::is_standard_layout<PathsArgs<PrevGather>>::value, "PathsArgs: the gathered batch comes last");

// test-only stage: explicit (iter, pixel) per path, in-place, no compaction
__global__ __launch_bounds__(kBlock) void k_shade_stage(SceneTables sc, int trace_depth, int depth, int n,
                                                        const int32_t* __restrict__ iter,
                                                        const int32_t* __restrict__ pixel, ptd::HitBuf hits,
                                                        ptd::PathBuf paths, int32_t* __restrict__ alive) {
  extern __shared__ float4 lds_raw[];
  char* lds = reinterpret_cast<char*>(lds_raw);
  const ShadeLds L = shade_lds<false>(sc);
  stage16(lds + L.mats, sc.mats, mat_bytes(sc));
  __syncthreads();
  const ptd::Mat* mats = reinterpret_cast<const ptd::Mat*>(lds + L.mats);
  const int64_t HS = hits.stride;
  for (int at = blockIdx.x * blockDim.x + threadIdx.x; at < n; at += gridDim.x * blockDim.x) {
    const PathRec pr = path_load(paths, at);
    ShadeIO s;
    s.o = pr.o;
    s.d = pr.d;
    s.c = pr.c;
    s.alive = false;
    const Bounce bo = shade_decide(mats, trace_depth, depth, iter_hash(iter[at], depth) ^ utilhash((uint32_t)pixel[at]), hits.t[at], hits.mat[at], s);
    // the stage reports the bounce ray whenever one is sampled (also at the last depth), like the reference
    if (bo.kind) shade_bounce(bo, mk(hits.n[at], hits.n[HS + at], hits.n[2 * HS + at]),
                              mk(hits.p[at], hits.p[HS + at], hits.p[2 * HS + at]), s);
    path_store(paths, at, s.o, s.d, s.c, pr.tag);
    alive[at] = s.alive ? 1 : 0;
  }
}

#include "pt_features.inc"
#include "pt_output.inc"
#include "pt_launch.inc"
const KernelApi kApi = {
#if PT_ARITH == 0
    "exact",
#elif PT_ARITH == 1
    "fma",
#else
    "fast",
#endif
    launch_generate, launch_primary, launch_intersect, launch_shade, launch_collect, launch_count_stats,
    launch_preview, launch_save_u8, launch_shade_stage, lds_table_limit, resident_blocks_per_cu, launch_ieee_check, launch_paths,
    launch_collect_conv, launch_features, kFast ? 1 : 0, launch_intersect_grid, launch_collect_stream, launch_paths_gather,
    launch_collect_stream_planes, launch_fast_math_check};

}  // namespace
}  // namespace PT_NS

const KernelApi* PT_API_FN() { return &PT_NS::kApi; }

#if defined(PT_WALK_STATS) && PT_ARITH == 2
}  // namespace ptk
// diagnostic builds only: the fast build's counters since the last call (read and reset)
extern "C" int pt_debug_walk_stats(unsigned long long* out) {
  unsigned long long zero[16] = {0};
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ptk::arith_fast::g_walk_stats), sizeof(zero)) != hipSuccess) return -1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(ptk::arith_fast::g_walk_stats), zero, sizeof(zero)) != hipSuccess) return -1;
  return 16;
}
namespace ptk {
#endif

}  // namespace ptk
