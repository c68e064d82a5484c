// pt_adaptive.hip — the kernels of adaptive sampling (include/pt_amd.h pt_adaptive_round) and their launchers.
//
// A translation unit of its own, compiled ONCE with -ffp-contract=off like pt_noise.hip: key, merge and resolve are specified as
// separate IEEE float32 operations (pt_adaptive.h), the selection works on the keys' bit patterns.  All of it is streaming and
// memory-bound; nothing synchronises with the host, and the only atomics are integer adds on histogram bins
// and on the threshold selection's count.
//
//   k_adaptive_key      one thread per tile pixel: 9 taps of plane 0's w and of the counts, 4 B out.
//   k_adaptive_hist     radix select, pass P = 0, 1, 2 over bits 31..21, 20..10, 9..0 of the key: a workgroup of 256 threads owns 1024
//                       consecutive pixels, counts those whose higher bits equal the prefix found so far in an LDS histogram and
//                       flushes its non-empty bins with integer atomics.
//   k_adaptive_pick     one workgroup: walks the pass's bins from the top (a suffix scan, 8 bins per thread) to the bin that holds
//                       the m-th largest key; leaves the longer prefix and the rank inside the bin in device memory.  After pass 2
//                       the prefix is the threshold key tau and the rank is r, the number of pixels equal to tau to take.
//   k_adaptive_count    per 1024-pixel block: pixels with key > tau, pixels with key == tau.
//   k_adaptive_above    selection by threshold: per 1024-pixel block, pixels with key > thr, added to one word with an integer atomic;
//   k_adaptive_threshold  one thread: (tau, r) := the cut under the threshold (pt_adaptive.h threshold_cut), m = min(above, cap).
//   k_adaptive_scan     one workgroup: the exclusive scan of both counts over the blocks.
//   k_adaptive_scatter  a pixel with a > pixels above tau and e pixels equal to tau in front of it (tile order) is taken when its key
//                       is above tau, or equal with e < r, and lands at list[a + min(e, r)]: ascending tile index, ties to the smaller
//                       index.  Ranks: ballot + mbcnt inside a wave, wave and row offsets through LDS.
//   k_adaptive_merge    one thread per list entry (pt_adaptive.h merge_pixel).
//   k_adaptive_partial  the fold's frame statistic over ALL tile pixels: one double per PT_NOISE_PIXELS_PER_PARTIAL consecutive
//                       pixels, k_noise_fold's tree; k_noise_reduce (pt_noise.hip) adds them in index order.
//   k_adaptive_resolve  one thread per pixel: S / (float)T_p.
#include <hip/hip_runtime.h>

#include "pt_adaptive.h"
#include "pt_internal.h"

namespace {
using ptad::Cnt;
using ptnz::V4;
constexpr int kBlock = 256;
constexpr int kPerBlock = 1024;  // pixels of a workgroup in the selection passes
constexpr int kPerThread = kPerBlock / kBlock;
constexpr int kWaves = kBlock / 64;
constexpr int kBins = 2048;
static_assert(kPerBlock == PT_NOISE_PIXELS_PER_PARTIAL, "k_adaptive_partial owns one partial sum per workgroup");
static_assert(kBins == kBlock * 8, "k_adaptive_pick: 8 bins per thread");

// The select's words in device memory
struct Sel {
  // While the passes run: the bits of tau found so far (the passes' bins, in place), and the rank (1-based) of the key looked for among
  // the keys that share the prefix.  Pass 2 leaves both words zero, and the selection by threshold keeps its two counts there (so the
  // workspace is as large as it was): pixels whose key exceeds thr, and min(above, cap), the list's length.
  union {
    uint32_t prefix, above;
  };
  union {
    uint32_t rank, m;
  };
  uint32_t tau, r;  // after pass 2: prefix and rank under their final names
};
static_assert(sizeof(Sel) == 16, "pt_adaptive_select_bytes, pt_adaptive_select_result");

__device__ __forceinline__ int pass_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__device__ __forceinline__ uint32_t pass_bin(uint32_t key, int pass) { return pass == 0 ? key >> 21 : pass == 1 ? (key >> 10) & 0x7ffu : key & 0x3ffu; }
// the bits above the pass's bin field agree with the prefix (pass 0: every key)
__device__ __forceinline__ bool pass_match(uint32_t key, uint32_t prefix, int pass) {
  return pass == 0 || (pass == 1 ? (key >> 21) == (prefix >> 21) : (key >> 10) == (prefix >> 10));
}

__global__ __launch_bounds__(kBlock) void k_adaptive_key(int W, int R, const V4* __restrict__ plane0, const Cnt* __restrict__ cnt,
                                                         uint32_t* __restrict__ key) {
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= (size_t)W * R) return;
  const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
  key[p] = ptad::key_pixel(x, y, W, R, plane0, cnt);
}

__global__ __launch_bounds__(kBlock) void k_adaptive_init_counts(size_t npix, Cnt* __restrict__ cnt, Cnt value) {
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p < npix) cnt[p] = value;
}

__global__ __launch_bounds__(kBlock) void k_adaptive_hist(size_t npix, const uint32_t* __restrict__ key, const Sel* __restrict__ sel, int pass,
                                                          uint32_t* __restrict__ hist) {
  __shared__ uint32_t bins[kBins];
  for (int i = threadIdx.x; i < kBins; i += kBlock) bins[i] = 0u;
  __syncthreads();
  const uint32_t prefix = pass == 0 ? 0u : sel->prefix;
  const size_t base = (size_t)blockIdx.x * kPerBlock + threadIdx.x;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const size_t p = base + (size_t)j * kBlock;
    if (p < npix) {
      const uint32_t k = key[p];
      if (pass_match(k, prefix, pass)) atomicAdd(&bins[pass_bin(k, pass)], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kBins; i += kBlock) {
    const uint32_t c = bins[i];
    if (c) atomicAdd(&hist[i], c);
  }
}

// Exclusive scan of one value per thread over the workgroup, in thread order; *total = the sum.  (two barriers; `tmp` holds kWaves + 1 words)
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

__global__ __launch_bounds__(kBlock) void k_adaptive_pick(const uint32_t* __restrict__ hist, Sel* __restrict__ sel, int pass, uint32_t m) {
  __shared__ uint32_t tmp[kWaves + 1];
  // thread t owns the bins kBins - 1 - 8 t downwards: thread order = descending key order
  const int top = kBins - 1 - 8 * (int)threadIdx.x;
  uint32_t c[8], mine = 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) c[i] = hist[top - i], mine += c[i];
  uint32_t total;
  uint32_t above = block_exclusive_scan(mine, tmp, &total);  // keys in the bins above this thread's
  const uint32_t rank = pass == 0 ? m : sel->rank;           // 1 <= rank <= total by construction
  const uint32_t prefix = pass == 0 ? 0u : sel->prefix;
  __syncthreads();  // every thread has read sel before one of them writes it
  if (rank > above && rank <= above + mine) {  // exactly one thread
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (rank > above && rank <= above + c[i]) {
        const uint32_t p = prefix | (uint32_t)(top - i) << pass_shift(pass);
        sel->prefix = pass == 2 ? 0u : p, sel->rank = pass == 2 ? 0u : rank - above;  // (after pass 2: Sel::above and Sel::m, from zero)
        sel->tau = p, sel->r = rank - above;
      }
      above += c[i];
    }
  }
}

struct Pair {
  uint32_t gt, eq;
};

__global__ __launch_bounds__(kBlock) void k_adaptive_count(size_t npix, const uint32_t* __restrict__ key, const Sel* __restrict__ sel,
                                                           Pair* __restrict__ per_block) {
  __shared__ uint32_t wave_gt[kWaves], wave_eq[kWaves];
  const uint32_t tau = sel->tau;
  const size_t base = (size_t)blockIdx.x * kPerBlock + threadIdx.x;
  uint32_t gt = 0u, eq = 0u;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const size_t p = base + (size_t)j * kBlock;
    if (p < npix) {
      const uint32_t k = key[p];
      gt += k > tau ? 1u : 0u, eq += k == tau ? 1u : 0u;
    }
  }
  for (int off = 32; off > 0; off >>= 1) gt += __shfl_down(gt, off, 64), eq += __shfl_down(eq, off, 64);
  if ((threadIdx.x & 63) == 0) wave_gt[threadIdx.x >> 6] = gt, wave_eq[threadIdx.x >> 6] = eq;
  __syncthreads();
  if (threadIdx.x == 0) {
    Pair s{0u, 0u};
    for (int w = 0; w < kWaves; ++w) s.gt += wave_gt[w], s.eq += wave_eq[w];
    per_block[blockIdx.x] = s;
  }
}

// Selection by threshold, after the picks for rank `cap`: sel->above += the block's pixels whose key exceeds thr (an integer atomic: the
// sum is the same in any order).
__global__ __launch_bounds__(kBlock) void k_adaptive_above(size_t npix, const uint32_t* __restrict__ key, uint32_t thr, Sel* __restrict__ sel) {
  __shared__ uint32_t wave_n[kWaves];
  const size_t base = (size_t)blockIdx.x * kPerBlock + threadIdx.x;
  uint32_t n = 0u;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const size_t p = base + (size_t)j * kBlock;
    if (p < npix) n += ptad::above_threshold(key[p], thr) ? 1u : 0u;
  }
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0u;
    for (int w = 0; w < kWaves; ++w) s += wave_n[w];
    if (s) atomicAdd(&sel->above, s);
  }
}
// ... and one thread: the cut under the threshold (pt_adaptive.h threshold_cut) for count, scan and scatter, and the list's length.
__global__ void k_adaptive_threshold(Sel* __restrict__ sel, uint32_t thr, uint32_t cap) {
  const ptad::Cut c = ptad::threshold_cut(sel->tau, sel->r, thr);
  sel->tau = c.tau, sel->r = c.r;
  sel->m = ptad::threshold_length(sel->above, cap);
}

// per_block[b] := the counts of the blocks in front of b.  One workgroup, kBlock blocks per pass, the running sums carried along.
__global__ __launch_bounds__(kBlock) void k_adaptive_scan(int blocks, Pair* __restrict__ per_block) {
  __shared__ uint32_t tmp[kWaves + 1];
  uint32_t carry_gt = 0u, carry_eq = 0u;
  for (int first = 0; first < blocks; first += kBlock) {
    const int b = first + (int)threadIdx.x;
    const Pair v = b < blocks ? per_block[b] : Pair{0u, 0u};
    uint32_t total_gt, total_eq;
    const uint32_t gt = block_exclusive_scan(v.gt, tmp, &total_gt);
    const uint32_t eq = block_exclusive_scan(v.eq, tmp, &total_eq);
    if (b < blocks) per_block[b] = Pair{carry_gt + gt, carry_eq + eq};
    carry_gt += total_gt, carry_eq += total_eq;
  }
}

__global__ __launch_bounds__(kBlock) void k_adaptive_scatter(size_t npix, const uint32_t* __restrict__ key, const Sel* __restrict__ sel,
                                                             const Pair* __restrict__ block_before, uint32_t m, int32_t* __restrict__ list) {
  __shared__ uint32_t cnt_gt[kPerThread][kWaves], cnt_eq[kPerThread][kWaves];  // pixel order inside the block: row j, then wave, then lane
  const uint32_t tau = sel->tau, r = sel->r;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t base = (size_t)blockIdx.x * kPerBlock + threadIdx.x;
  bool gt[kPerThread], eq[kPerThread];
  uint32_t rank_gt[kPerThread], rank_eq[kPerThread];
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const size_t p = base + (size_t)j * kBlock;
    const uint32_t k = p < npix ? key[p] : 0u;
    gt[j] = p < npix && k > tau, eq[j] = p < npix && k == tau;
    const unsigned long long mg = __ballot(gt[j]), me = __ballot(eq[j]);
    rank_gt[j] = __builtin_amdgcn_mbcnt_hi((uint32_t)(mg >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mg, 0u));
    rank_eq[j] = __builtin_amdgcn_mbcnt_hi((uint32_t)(me >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)me, 0u));
    if (lane == 0) cnt_gt[j][wave] = (uint32_t)__popcll(mg), cnt_eq[j][wave] = (uint32_t)__popcll(me);
  }
  __syncthreads();
  const Pair before = block_before[blockIdx.x];
  uint32_t a = before.gt, e = before.eq;  // pixels above / equal to tau in front of row j's wave `wave`
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    uint32_t aj = a, ej = e;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) aj += cnt_gt[j][w], ej += cnt_eq[j][w];
      a += cnt_gt[j][w], e += cnt_eq[j][w];
    }
    const uint32_t above = aj + rank_gt[j], equal = ej + rank_eq[j];
    const bool take = gt[j] || (eq[j] && equal < r);
    const uint32_t at = above + (equal < r ? equal : r);
    if (take && at < m) list[at] = (int32_t)(base + (size_t)j * kBlock);  // (at < m by construction; the list holds m entries)
  }
}

__global__ __launch_bounds__(kBlock) void k_adaptive_merge(size_t npix, int m, const int32_t* __restrict__ list, const float* __restrict__ Sw, float nf,
                                                           int group_iters, float* __restrict__ S, V4* __restrict__ planes, Cnt* __restrict__ cnt) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < (size_t)m && (size_t)list[i] < npix) ptad::merge_pixel(i, npix, list, Sw, nf, group_iters, S, planes, cnt);  // (an entry outside the tile writes nothing)
}

__global__ __launch_bounds__(kBlock) void k_adaptive_partial(size_t npix, const V4* __restrict__ plane0, double* __restrict__ partial) {
  __shared__ double wave_sum[kWaves];
  const size_t base = (size_t)blockIdx.x * kPerBlock + threadIdx.x;
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const size_t i = base + (size_t)j * kBlock;
    if (i < npix) sum += (double)plane0[i].w;
  }
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = wave_sum[0];
    for (int w = 1; w < kWaves; ++w) s += wave_sum[w];
    partial[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kBlock) void k_adaptive_resolve(size_t npix, const float* __restrict__ S, const Cnt* __restrict__ cnt, int32_t T,
                                                             float* __restrict__ out) {
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p < npix) ptad::resolve_pixel(p, S, cnt, T, out);
}

unsigned blocks_of(size_t n, int per) { return (unsigned)((n + per - 1) / per); }
int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : pt_fail("%s: launch failed: %s", who, hipGetErrorString(e));
}

// the workspace of a selection (pt_adaptive_select_bytes): keys | three histograms | Sel | one Pair per block
struct Workspace {
  uint32_t* key;
  uint32_t* hist;
  Sel* sel;
  Pair* per_block;
};
Workspace carve(void* ws, size_t npix) {
  Workspace w;
  w.key = static_cast<uint32_t*>(ws);
  w.hist = w.key + ((npix + 3) & ~(size_t)3);
  w.sel = reinterpret_cast<Sel*>(w.hist + 3 * kBins);
  w.per_block = reinterpret_cast<Pair*>(w.sel + 1);
  return w;
}
}  // namespace

// pt_internal.h
size_t pt_adaptive_select_bytes(size_t pixels) {
  return 4 * ((pixels + 3) & ~(size_t)3) + 4 * 3 * kBins + sizeof(Sel) + sizeof(Pair) * ((pixels + kPerBlock - 1) / kPerBlock);
}

int pt_adaptive_init_counts_launch(hipStream_t stream, int pixels, void* counts_dev, int iters, int groups) {
  if (pixels <= 0 || !counts_dev) return pt_fail("pt_adaptive_round: bad argument");
  hipLaunchKernelGGL(k_adaptive_init_counts, dim3(blocks_of((size_t)pixels, kBlock)), dim3(kBlock), 0, stream, (size_t)pixels, static_cast<Cnt*>(counts_dev),
                     Cnt{iters, groups});
  return launched("pt_adaptive_round");
}

// The selection's launches; thr == nullptr: the top m, else the pixels above *thr, the `m` with the largest keys at the most.
// noise_dev == nullptr: the keys are in the workspace already (pt_adaptive_select_keys), and nothing else of the pixels is read.
static int select_launches(const char* who, hipStream_t stream, int w, int rows, const float* noise_dev, const void* counts_dev, int m, const uint32_t* thr,
                           void* workspace_dev, int32_t* list_dev) {
  const size_t npix = (size_t)w * rows;
  if (w <= 0 || rows <= 0 || npix > ((size_t)1 << 30) || m < 1 || (size_t)m > npix || !noise_dev != !counts_dev || !workspace_dev || !list_dev)
    return pt_fail("%s: bad argument", who);
  const Workspace ws = carve(workspace_dev, npix);
  const unsigned blocks = blocks_of(npix, kPerBlock);
  if (hipMemsetAsync(ws.hist, 0, 4 * 3 * kBins + sizeof(Sel), stream) != hipSuccess) return pt_fail("%s: hipMemsetAsync failed", who);
  if (noise_dev)
    hipLaunchKernelGGL(k_adaptive_key, dim3(blocks_of(npix, kBlock)), dim3(kBlock), 0, stream, w, rows, reinterpret_cast<const V4*>(noise_dev),
                       static_cast<const Cnt*>(counts_dev), ws.key);
  for (int pass = 0; pass < 3; ++pass) {
    hipLaunchKernelGGL(k_adaptive_hist, dim3(blocks), dim3(kBlock), 0, stream, npix, ws.key, ws.sel, pass, ws.hist + pass * kBins);
    hipLaunchKernelGGL(k_adaptive_pick, dim3(1), dim3(kBlock), 0, stream, ws.hist + pass * kBins, ws.sel, pass, (uint32_t)m);
  }
  if (thr) {
    hipLaunchKernelGGL(k_adaptive_above, dim3(blocks), dim3(kBlock), 0, stream, npix, ws.key, *thr, ws.sel);
    hipLaunchKernelGGL(k_adaptive_threshold, dim3(1), dim3(1), 0, stream, ws.sel, *thr, (uint32_t)m);
  }
  hipLaunchKernelGGL(k_adaptive_count, dim3(blocks), dim3(kBlock), 0, stream, npix, ws.key, ws.sel, ws.per_block);
  hipLaunchKernelGGL(k_adaptive_scan, dim3(1), dim3(kBlock), 0, stream, (int)blocks, ws.per_block);
  hipLaunchKernelGGL(k_adaptive_scatter, dim3(blocks), dim3(kBlock), 0, stream, npix, ws.key, ws.sel, ws.per_block, (uint32_t)m, list_dev);
  return launched(who);
}

int pt_adaptive_select_launch(hipStream_t stream, int w, int rows, const float* noise_dev, const void* counts_dev, int m, void* workspace_dev,
                              int32_t* list_dev) {
  return select_launches("pt_adaptive_select", stream, w, rows, noise_dev, counts_dev, m, nullptr, workspace_dev, list_dev);
}

int pt_adaptive_select_threshold_launch(hipStream_t stream, int w, int rows, const float* noise_dev, const void* counts_dev, float threshold, int cap,
                                        void* workspace_dev, int32_t* list_dev) {
  if (!std::isfinite(threshold) || threshold < 0.0f) return pt_fail("pt_adaptive_select_threshold: bad argument");
  const uint32_t thr = ptad::threshold_bits(threshold);
  return select_launches("pt_adaptive_select_threshold", stream, w, rows, noise_dev, counts_dev, cap, &thr, workspace_dev, list_dev);
}

int pt_adaptive_select_threshold_keys_launch(hipStream_t stream, int w, int rows, float threshold, int cap, void* workspace_dev, int32_t* list_dev) {
  if (!std::isfinite(threshold) || threshold < 0.0f) return pt_fail("pt_adaptive_select_threshold: bad argument");
  const uint32_t thr = ptad::threshold_bits(threshold);
  return select_launches("pt_adaptive_select_threshold", stream, w, rows, nullptr, nullptr, cap, &thr, workspace_dev, list_dev);
}

uint32_t* pt_adaptive_select_keys(void* workspace_dev, size_t pixels) { return carve(workspace_dev, pixels).key; }

const uint32_t* pt_adaptive_select_result(const void* workspace_dev, size_t pixels) { return &carve(const_cast<void*>(workspace_dev), pixels).sel->above; }

int pt_adaptive_merge_launch(hipStream_t stream, int pixels, float* rgb_sum_dev, void* noise_state_dev, void* counts_dev, const int32_t* list_dev, int m,
                             const float* group_sum_dev, int group_iters) {
  if (pixels <= 0 || pixels > (1 << 30) || m < 1 || m > pixels || group_iters < 1 || !rgb_sum_dev || !noise_state_dev || !counts_dev || !list_dev ||
      !group_sum_dev)
    return pt_fail("pt_adaptive_merge: bad argument");
  V4* planes = static_cast<V4*>(noise_state_dev);
  double* partial = reinterpret_cast<double*>(planes + (size_t)PT_NOISE_PLANES * pixels);  // pt_noise_state_bytes
  const int blocks = (int)pt_noise_partials((size_t)pixels);
  hipLaunchKernelGGL(k_adaptive_merge, dim3(blocks_of((size_t)m, kBlock)), dim3(kBlock), 0, stream, (size_t)pixels, m, list_dev, group_sum_dev,
                     (float)group_iters, group_iters, rgb_sum_dev, planes, static_cast<Cnt*>(counts_dev));
  hipLaunchKernelGGL(k_adaptive_partial, dim3(blocks), dim3(kBlock), 0, stream, (size_t)pixels, planes, partial);
  if (launched("pt_adaptive_merge")) return -1;
  return pt_noise_reduce_launch(stream, blocks, partial, partial + blocks);
}

int pt_adaptive_resolve_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const void* counts_dev, int iters, float* rgb_avg_dev) {
  if (pixels <= 0 || !rgb_sum_dev || !rgb_avg_dev || (!counts_dev && iters < 1)) return pt_fail("pt_resolve: bad argument");
  hipLaunchKernelGGL(k_adaptive_resolve, dim3(blocks_of((size_t)pixels, kBlock)), dim3(kBlock), 0, stream, (size_t)pixels, rgb_sum_dev,
                     static_cast<const Cnt*>(counts_dev), iters, rgb_avg_dev);
  return launched("pt_resolve");
}

// pt_internal.h: what both forms of the selection refuse
int pt_adaptive_check_select(const char* who, int w, int rows, const float* noise_planes, const int32_t* counts, int m, const int32_t* list) {
  if (w <= 0 || rows <= 0 || rows >= 32768 || (int64_t)w * rows > (1ll << 30) || !noise_planes || !counts || !list)
    return pt_fail("%s: bad argument", who);
  if (m < 1 || (int64_t)m > (int64_t)w * rows) return pt_fail("%s: a list of %d out of %lld pixels", who, m, (long long)w * rows);
  for (int64_t p = 0; p < (int64_t)w * rows; ++p)
    if (counts[2 * p] < 1) return pt_fail("%s: pixel %lld has no iterations (counts are T_p >= 1, M_p)", who, (long long)p);
  return 0;
}

extern "C" int pt_adaptive_select_host(int w, int rows, const float* noise_planes, const int32_t* counts, int m, int32_t* list) {
  if (pt_adaptive_check_select("pt_adaptive_select_host", w, rows, noise_planes, counts, m, list)) return -1;
  ptad::select_host(w, rows, noise_planes, counts, m, list);
  return 0;
}

int pt_adaptive_check_threshold(const char* who, float threshold) {
  return std::isfinite(threshold) && threshold >= 0.0f ? 0 : pt_fail("%s: threshold %g is not finite and >= 0", who, (double)threshold);
}

extern "C" int pt_adaptive_select_threshold_host(int w, int rows, const float* noise_planes, const int32_t* counts, float threshold, int cap, int32_t* list,
                                                 int* above, int* m) {
  if (pt_adaptive_check_select("pt_adaptive_select_threshold_host", w, rows, noise_planes, counts, cap, list)) return -1;
  if (pt_adaptive_check_threshold("pt_adaptive_select_threshold_host", threshold)) return -1;
  if (!above || !m) return pt_fail("pt_adaptive_select_threshold_host: bad argument");
  ptad::select_threshold_host(w, rows, noise_planes, counts, threshold, cap, list, above, m);
  return 0;
}

extern "C" int pt_adaptive_merge_host(int pixels, float* rgb_sum, float* planes, int32_t* counts, const int32_t* list, int m, const float* group_sum,
                                      int group_iters, double* sse) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum || !planes || !counts || !list || !group_sum) return pt_fail("pt_adaptive_merge_host: bad argument");
  if (m < 1 || m > pixels || group_iters < 1) return pt_fail("pt_adaptive_merge_host: a list of %d out of %d pixels, a group of %d iterations", m, pixels, group_iters);
  std::vector<uint8_t> seen((size_t)pixels, 0);
  for (int i = 0; i < m; ++i) {
    if (list[i] < 0 || list[i] >= pixels || seen[(size_t)list[i]]) return pt_fail("pt_adaptive_merge_host: list[%d] = %d is outside the tile or repeated", i, list[i]);
    seen[(size_t)list[i]] = 1;
    if (counts[2 * (size_t)list[i]] < 1 || counts[2 * (size_t)list[i] + 1] < 1)
      return pt_fail("pt_adaptive_merge_host: pixel %d has no folded group (counts are T_p >= 1, M_p >= 1)", list[i]);
  }
  const double s = ptad::merge_host((size_t)pixels, rgb_sum, planes, counts, list, m, group_sum, group_iters);
  if (sse) *sse = s;
  return 0;
}
