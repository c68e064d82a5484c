// pt_group_select.hip — the kernels a group of contexts adds to adaptive sampling by threshold (pt_group_select.h) and their launchers.
//
// Compiled once with -ffp-contract=off like pt_adaptive.hip, whose key arithmetic k_group_key runs.  Streaming and memory-bound;
// nothing synchronises with the host; the only atomics are integer adds on per-part counters in LDS, never used to order entries.
//
//   k_group_pack        one thread per tile pixel: {w_p, T_p} from plane 0 and the count plane, 8 B out.
//   k_group_key         one thread per frame pixel: ptad::key_pixel on the packed frame, 4 B out (into the selection's workspace).
//   k_group_offsets     one thread per list entry: tile index -> frame offset on a striped tile.
//   k_partition_count   a workgroup of 256 threads owns 1024 consecutive list entries: entries per part.
//   k_partition_scan    one workgroup: per part, the exclusive scan of the counts over the blocks; the parts' lengths and their
//                       offsets in the output; the words the host reads back.
//   k_partition_scatter entry j of the list, owned by part i with e entries of part i in front of it, lands at parts[offset_i + e]:
//                       input order.  Ranks: one ballot + mbcnt per part inside a wave, wave and row counts through LDS.
// The list's length is read from the selection's words on the device, so the three launches follow the selection without a
// synchronise; blocks behind the list's end count and write nothing.
#include <hip/hip_runtime.h>

#include <vector>

#include "pt_group_select.h"
#include "pt_internal.h"

namespace {
using ptad::Cnt;
using ptgs::kMaxParts;
using ptgs::Packed;
using ptnz::V4;
constexpr int kBlock = 256;
constexpr int kPerBlock = 1024;
constexpr int kPerThread = kPerBlock / kBlock;
constexpr int kWaves = kBlock / 64;

__global__ __launch_bounds__(kBlock) void k_group_pack(size_t npix, const V4* __restrict__ plane0, const Cnt* __restrict__ cnt, Packed* __restrict__ out) {
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p < npix) out[p] = ptgs::pack_pixel(p, plane0, cnt);
}

__global__ __launch_bounds__(kBlock) void k_group_key(int W, int H, const Packed* __restrict__ frame, uint32_t* __restrict__ key) {
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= (size_t)W * H) return;
  const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
  key[p] = ptgs::key_packed(x, y, W, H, frame);
}

__global__ __launch_bounds__(kBlock) void k_group_offsets(int m, const int32_t* __restrict__ list, int stripe, int gap, int32_t* __restrict__ out) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (i < m) out[i] = ptgs::stripe_offset(list[i], stripe, gap);
}

__global__ __launch_bounds__(kBlock) void k_partition_count(const int32_t* __restrict__ list, const uint32_t* __restrict__ sel, int W, int n,
                                                            uint32_t capacity, uint32_t* __restrict__ per_block) {
  __shared__ uint32_t part[kMaxParts];
  if ((int)threadIdx.x < n) part[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t m = sel[1] < capacity ? sel[1] : capacity;  // (m <= capacity by construction; the list holds `capacity` entries)
  const uint32_t base = blockIdx.x * kPerBlock + threadIdx.x;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const uint32_t i = base + (uint32_t)j * kBlock;
    if (i < m) atomicAdd(&part[ptgs::owner_of(list[i], W, n)], 1u);
  }
  __syncthreads();
  if ((int)threadIdx.x < n) per_block[(size_t)blockIdx.x * n + threadIdx.x] = part[threadIdx.x];
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

// per_block[b][i] := the entries of part i in the blocks in front of b; offset[i] := the entries of the parts in front of part i;
// result := {above, m, m_0 .. m_(n-1)}.
__global__ __launch_bounds__(kBlock) void k_partition_scan(int blocks, int n, uint32_t* __restrict__ per_block, uint32_t* __restrict__ offset,
                                                           const uint32_t* __restrict__ sel, uint32_t* __restrict__ result) {
  __shared__ uint32_t tmp[kWaves];
  __shared__ uint32_t length[kMaxParts];
  for (int i = 0; i < n; ++i) {
    uint32_t carry = 0u;
    for (int first = 0; first < blocks; first += kBlock) {
      const int b = first + (int)threadIdx.x;
      const uint32_t v = b < blocks ? per_block[(size_t)b * n + i] : 0u;
      uint32_t total;
      const uint32_t before = block_exclusive_scan(v, tmp, &total);
      if (b < blocks) per_block[(size_t)b * n + i] = carry + before;
      carry += total;
    }
    if (threadIdx.x == 0) length[i] = carry;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    result[0] = sel[0], result[1] = sel[1];
    uint32_t sum = 0u;
    for (int i = 0; i < n; ++i) offset[i] = sum, result[2 + i] = length[i], sum += length[i];
  }
}

__global__ __launch_bounds__(kBlock) void k_partition_scatter(const int32_t* __restrict__ list, const uint32_t* __restrict__ sel, int W, int n,
                                                              const uint32_t* __restrict__ block_before, const uint32_t* __restrict__ offset,
                                                              uint32_t capacity, int32_t* __restrict__ parts) {
  __shared__ uint32_t count[kPerThread][kWaves][kMaxParts];  // entry order inside the block: row j, then wave, then lane
  const uint32_t m = sel[1] < capacity ? sel[1] : capacity;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t base = blockIdx.x * kPerBlock + threadIdx.x;
  int32_t f[kPerThread];
  int owner[kPerThread];
  uint32_t rank[kPerThread];
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const uint32_t i = base + (uint32_t)j * kBlock;
    const bool valid = i < m;
    f[j] = valid ? list[i] : 0;
    owner[j] = valid ? ptgs::owner_of(f[j], W, n) : -1;
    rank[j] = 0u;
    for (int o = 0; o < n; ++o) {  // (uniform: every lane runs every part)
      const unsigned long long mask = __ballot(owner[j] == o);
      if (owner[j] == o) rank[j] = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
      if (lane == 0) count[j][wave][o] = (uint32_t)__popcll(mask);
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    if (owner[j] < 0) continue;
    uint32_t e = block_before[(size_t)blockIdx.x * n + owner[j]] + rank[j];
    for (int jj = 0; jj <= j; ++jj)
      for (int w = 0; w < kWaves; ++w)
        if (jj < j || w < wave) e += count[jj][w][owner[j]];
    const uint32_t at = offset[owner[j]] + e;
    if (at < capacity) parts[at] = ptgs::tile_index(f[j], W, n);  // (at < m <= capacity by construction)
  }
}

unsigned blocks_of(size_t n, int per) { return (unsigned)((n + per - 1) / per); }
int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : pt_fail("%s: launch failed: %s", who, hipGetErrorString(e));
}
}  // namespace

// pt_internal.h
int pt_group_pack_launch(hipStream_t stream, int pixels, const float* noise_dev, const void* counts_dev, void* packed_dev) {
  if (pixels <= 0 || !noise_dev || !counts_dev || !packed_dev) return pt_fail("pt_group_pack: bad argument");
  hipLaunchKernelGGL(k_group_pack, dim3(blocks_of((size_t)pixels, kBlock)), dim3(kBlock), 0, stream, (size_t)pixels, reinterpret_cast<const V4*>(noise_dev),
                     static_cast<const Cnt*>(counts_dev), static_cast<Packed*>(packed_dev));
  return launched("pt_group_pack");
}

int pt_group_keys_launch(hipStream_t stream, int w, int rows, const void* packed_dev, uint32_t* key_dev) {
  const size_t npix = (size_t)w * rows;
  if (w <= 0 || rows <= 0 || npix > ((size_t)1 << 30) || !packed_dev || !key_dev) return pt_fail("pt_group_keys: bad argument");
  hipLaunchKernelGGL(k_group_key, dim3(blocks_of(npix, kBlock)), dim3(kBlock), 0, stream, w, rows, static_cast<const Packed*>(packed_dev), key_dev);
  return launched("pt_group_keys");
}

int pt_group_offsets_launch(hipStream_t stream, const int32_t* list_dev, int m, int stripe, int gap, int32_t* offsets_dev) {
  if (m < 1 || stripe < 1 || gap < 0 || !list_dev || !offsets_dev) return pt_fail("pt_group_offsets: bad argument");
  hipLaunchKernelGGL(k_group_offsets, dim3(blocks_of((size_t)m, kBlock)), dim3(kBlock), 0, stream, m, list_dev, stripe, gap, offsets_dev);
  return launched("pt_group_offsets");
}

// the workspace of a partition: one count per block and part | one offset per part
size_t pt_group_partition_bytes(size_t max_entries, int n) { return 4 * ((size_t)blocks_of(max_entries, kPerBlock) * n + n); }

int pt_group_partition_launch(hipStream_t stream, int w, int n, const int32_t* list_dev, const uint32_t* select_result_dev, int max_entries,
                              void* workspace_dev, int32_t* parts_dev, uint32_t* result_dev) {
  if (w <= 0 || n < 1 || n > kMaxParts || max_entries < 1 || max_entries > (1 << 30) || !list_dev || !select_result_dev || !workspace_dev || !parts_dev ||
      !result_dev)
    return pt_fail("pt_group_partition: bad argument");
  const unsigned blocks = blocks_of((size_t)max_entries, kPerBlock);
  uint32_t* per_block = static_cast<uint32_t*>(workspace_dev);
  uint32_t* offset = per_block + (size_t)blocks * n;
  hipLaunchKernelGGL(k_partition_count, dim3(blocks), dim3(kBlock), 0, stream, list_dev, select_result_dev, w, n, (uint32_t)max_entries, per_block);
  hipLaunchKernelGGL(k_partition_scan, dim3(1), dim3(kBlock), 0, stream, (int)blocks, n, per_block, offset, select_result_dev, result_dev);
  hipLaunchKernelGGL(k_partition_scatter, dim3(blocks), dim3(kBlock), 0, stream, list_dev, select_result_dev, w, n, per_block, offset, (uint32_t)max_entries,
                     parts_dev);
  return launched("pt_group_partition");
}

int pt_group_partition_check(const char* who, int w, int h, int n, const int32_t* list, int m, const int32_t* parts, const int32_t* counts) {
  if (w <= 0 || h <= 0 || h >= 32768 || (int64_t)w * h > (1ll << 30)) return pt_fail("%s: a frame of %d x %d pixels is not supported", who, w, h);
  if (n < 1 || n > h || n > kMaxParts) return pt_fail("%s: %d contexts for %d rows: at least 1, at most a row each and at most %d", who, n, h, kMaxParts);
  if (m < 0 || (int64_t)m > (int64_t)w * h) return pt_fail("%s: a list of %d out of %lld pixels", who, m, (long long)w * h);
  if (!counts || (m > 0 && (!list || !parts))) return pt_fail("%s: null argument", who);
  for (int j = 0; j < m; ++j)
    if (list[j] < 0 || list[j] >= w * h || (j > 0 && list[j] <= list[j - 1]))
      return pt_fail("%s: list[%d] = %d is outside the frame or not above its predecessor", who, j, list[j]);
  return 0;
}

extern "C" int pt_group_partition_host(int w, int h, int n, const int32_t* list, int m, int32_t* parts, int32_t* counts) {
  if (pt_group_partition_check("pt_group_partition_host", w, h, n, list, m, parts, counts)) return -1;
  ptgs::partition_host(w, n, list, m, parts, counts);
  return 0;
}
