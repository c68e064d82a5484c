// pt_noise.hip — the kernels of the noise estimate (include/pt_amd.h pt_noise_fold) and their launcher.
//
// A translation unit of its own, compiled ONCE with -ffp-contract=off like pt_denoise.hip: the fold is specified as separate IEEE
// float32 operations (pt_noise.h), so there is nothing an arithmetic mode could change, and the path tracer's kernels
// (pt_kernels.hip) are not touched: the fold reads the SUM image between batches, k_collect knows nothing of it.
//
//   k_noise_fold    streaming, memory-bound: a workgroup of 256 threads owns PT_NOISE_PIXELS_PER_PARTIAL = 1024 consecutive tile
//                   pixels, a thread the pixels t, t + 256, t + 512, t + 768 of them (consecutive lanes, consecutive pixels: 1 KiB
//                   per wave and plane load).  Per pixel 12 B of S and 32 B of state in, 32 B of state out; the workgroup's
//                   estimates leave as ONE double (a fixed tree: shuffles inside a wave, then the four waves in order), no atomics.
//   k_noise_reduce  one workgroup: the partials pass through LDS 1024 at a time and thread 0 adds them in index order.
//   k_history_noise the noise estimate of the BLEND (pt_history_noise; the arithmetic is pt_history.h noise_pixel): k_noise_fold's shape
//                   over the planes a fold left, 32 B of state and (C, VC present) 32 B of history in, 4 B of W out per pixel, one
//                   double per workgroup from the same tree.
//   k_noise_fold_history  the two in one launch (pt_history_render_until): fold_pixel, then the estimate on the two words it just
//                   wrote, which never come back from memory; two doubles per workgroup.
#include <hip/hip_runtime.h>

#include "pt_history.h"
#include "pt_internal.h"
#include "pt_noise.h"

namespace {
using ptnz::Fold;
using ptnz::V4;
constexpr int kBlock = 256;
constexpr int kPerThread = PT_NOISE_PIXELS_PER_PARTIAL / kBlock;
constexpr int kWaves = kBlock / 64;
constexpr int kReduce = 1024;  // threads of k_noise_reduce = partials per pass through LDS
static_assert(PT_NOISE_PIXELS_PER_PARTIAL == 1024, "pt_internal.h pt_noise_partials");
static_assert(kPerThread * kBlock == PT_NOISE_PIXELS_PER_PARTIAL && kBlock % 64 == 0, "a workgroup owns exactly one partial sum");

__global__ __launch_bounds__(kBlock) void k_noise_fold(int npix, const float* __restrict__ S, V4* __restrict__ planes, Fold f,
                                                       double* __restrict__ partial) {
  __shared__ double wave_sum[kWaves];
  const size_t base = (size_t)blockIdx.x * PT_NOISE_PIXELS_PER_PARTIAL + threadIdx.x;
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const size_t i = base + (size_t)j * kBlock;
    if (i < (size_t)npix) sum += (double)ptnz::fold_pixel(i, (size_t)npix, S, planes, f);
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

// k_noise_fold's tree for one more kernel: shuffles inside a wave, then the four waves in order; thread 0 holds the sum.
__device__ __forceinline__ double block_sum(double sum, double* wave_sum) {
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
    s = wave_sum[0];
    for (int w = 1; w < kWaves; ++w) s += wave_sum[w];
  }
  return s;
}

using H4 = pthi::V4;
__global__ __launch_bounds__(kBlock) void k_history_noise(int npix, const V4* __restrict__ planes, float Tf, float Df, float samples,
                                                          const H4* __restrict__ C, const H4* __restrict__ VC, float* __restrict__ W,
                                                          double* __restrict__ partial) {
  __shared__ double wave_sum[kWaves];
  const size_t base = (size_t)blockIdx.x * PT_NOISE_PIXELS_PER_PARTIAL + threadIdx.x;
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const size_t i = base + (size_t)j * kBlock;
    if (i < (size_t)npix) {
      const float w = pthi::noise_pixel(i, (size_t)npix, planes, Tf, Df, samples, C, VC);
      W[i] = w;
      sum += (double)w;
    }
  }
  const double s = block_sum(sum, wave_sum);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(kBlock) void k_noise_fold_history(int npix, const float* __restrict__ S, V4* __restrict__ planes, Fold f, float samples,
                                                               const H4* __restrict__ C, const H4* __restrict__ VC, float* __restrict__ W,
                                                               double* __restrict__ partial, double* __restrict__ partial_blend) {
  __shared__ double wave_sum[2][kWaves];
  const size_t base = (size_t)blockIdx.x * PT_NOISE_PIXELS_PER_PARTIAL + threadIdx.x;
  const H4 zero{0.0f, 0.0f, 0.0f, 0.0f};
  double sum = 0.0, sum_blend = 0.0;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const size_t i = base + (size_t)j * kBlock;
    if (i < (size_t)npix) {
      V4 kept[2];
      sum += (double)ptnz::fold_pixel(i, (size_t)npix, S, planes, f, kept);
      const float w = pthi::noise_value(kept[0], kept[1], f.Tf, f.Df, samples, C ? C[i].w : 0.0f, VC ? VC[i] : zero);
      W[i] = w;
      sum_blend += (double)w;
    }
  }
  const double s = block_sum(sum, wave_sum[0]);
  const double sb = block_sum(sum_blend, wave_sum[1]);
  if (threadIdx.x == 0) partial[blockIdx.x] = s, partial_blend[blockIdx.x] = sb;
}

// The sum is one thread's: the order is the specification.  What is left to do is to keep that thread fed — the partials arrive
// kReduce at a time through LDS, the next chunk's loads are in flight while this one is added, and the chunk loop has a fixed trip
// count (the tail is padded with +0, which changes no bit of a sum of non-negative numbers) so that the LDS reads run ahead of the adds.
__global__ __launch_bounds__(kReduce) void k_noise_reduce(int count, const double* __restrict__ partial, double* __restrict__ sse) {
  __shared__ double stage[kReduce];
  double s = 0.0;
  double next = (int)threadIdx.x < count ? partial[threadIdx.x] : 0.0;
  for (int first = 0; first < count; first += kReduce) {
    stage[threadIdx.x] = next;
    __syncthreads();
    const int i = first + kReduce + (int)threadIdx.x;
    next = i < count ? partial[i] : 0.0;
    if (threadIdx.x == 0) {
#pragma unroll 16
      for (int k = 0; k < kReduce; ++k) s += stage[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *sse = s;
}

}  // namespace

// pt_internal.h.  Everything is checked before the first launch; no allocation, no synchronisation.
int pt_noise_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, void* state_dev, const Fold& f) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum_dev || !state_dev || !(f.nf >= 1.0f) || !(f.Tf >= f.nf))
    return pt_fail("pt_noise_fold: bad argument");
  V4* planes = static_cast<V4*>(state_dev);
  double* partial = reinterpret_cast<double*>(planes + (size_t)PT_NOISE_PLANES * pixels);
  const int blocks = (int)pt_noise_partials((size_t)pixels);
  hipLaunchKernelGGL(k_noise_fold, dim3(blocks), dim3(kBlock), 0, stream, pixels, rgb_sum_dev, planes, f, partial);
  return pt_noise_reduce_launch(stream, blocks, partial, partial + blocks);
}

// pt_internal.h: the second half of a fold on its own (the merge of pt_adaptive_round produces partial sums of the same kind)
int pt_noise_reduce_launch(hipStream_t stream, int count, const double* partial_dev, double* sse_dev) {
  hipLaunchKernelGGL(k_noise_reduce, dim3(1), dim3(kReduce), 0, stream, count, partial_dev, sse_dev);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pt_fail("pt_noise_fold: launch failed: %s", hipGetErrorString(e));
  return 0;
}

// pt_internal.h: out_dev holds pt_history_noise_bytes(pixels) bytes — the partial sums, the double they add up to, then W.
namespace {
bool bad_estimate(int pixels, const void* state_dev, float Tf, float Df, float samples, const void* current_dev, const void* current_var_dev, const void* out_dev) {
  return pixels <= 0 || pixels > (1 << 30) || !state_dev || !(Tf >= 2.0f) || !(Df >= Tf) || !(samples > 0.0f) || !current_dev != !current_var_dev || !out_dev;
}
}  // namespace
int pt_history_noise_launch(hipStream_t stream, int pixels, const void* state_dev, float Tf, float Df, float samples, const void* current_dev,
                            const void* current_var_dev, void* out_dev) {
  if (bad_estimate(pixels, state_dev, Tf, Df, samples, current_dev, current_var_dev, out_dev)) return pt_fail("pt_history_noise: bad argument");
  const int blocks = (int)pt_noise_partials((size_t)pixels);
  double* partial = static_cast<double*>(out_dev);
  hipLaunchKernelGGL(k_history_noise, dim3(blocks), dim3(kBlock), 0, stream, pixels, static_cast<const V4*>(state_dev), Tf, Df, samples,
                     static_cast<const H4*>(current_dev), static_cast<const H4*>(current_var_dev), pt_history_noise_plane(out_dev, (size_t)pixels), partial);
  return pt_noise_reduce_launch(stream, blocks, partial, partial + blocks);
}
int pt_noise_fold_history_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, void* state_dev, const Fold& f, float samples, const void* current_dev,
                                 const void* current_var_dev, void* out_dev) {
  if (!rgb_sum_dev || !(f.nf >= 1.0f) || !f.have_variance || bad_estimate(pixels, state_dev, f.Tf, f.Df, samples, current_dev, current_var_dev, out_dev))
    return pt_fail("pt_history_render_until: bad argument");
  V4* planes = static_cast<V4*>(state_dev);
  double* partial = reinterpret_cast<double*>(planes + (size_t)PT_NOISE_PLANES * pixels);
  double* partial_blend = static_cast<double*>(out_dev);
  const int blocks = (int)pt_noise_partials((size_t)pixels);
  hipLaunchKernelGGL(k_noise_fold_history, dim3(blocks), dim3(kBlock), 0, stream, pixels, rgb_sum_dev, planes, f, samples, static_cast<const H4*>(current_dev),
                     static_cast<const H4*>(current_var_dev), pt_history_noise_plane(out_dev, (size_t)pixels), partial, partial_blend);
  if (pt_noise_reduce_launch(stream, blocks, partial, partial + blocks)) return -1;
  return pt_noise_reduce_launch(stream, blocks, partial_blend, partial_blend + blocks);
}

// What the host and stage forms of the estimate refuse, in pt_history_capture_variance_host's order.
int pt_history_noise_check(const char* who, int pixels, const float* noise_planes, int groups, int64_t iters, float samples, const float* current_plane,
                           const float* current_var) {
  if (pixels <= 0 || pixels > (1 << 30) || !noise_planes) return pt_fail("%s: bad argument", who);
  if (pt_history_check_samples(who, samples)) return -1;
  if (groups < 2) return pt_fail("%s: %d group(s) folded; a variance needs at least 2 (pt_noise_fold after each group of iterations)", who, groups);
  if (iters < groups) return pt_fail("%s: %d groups cannot hold %lld iterations (every group holds at least one)", who, groups, (long long)iters);
  if (pt_history_check_fold_samples(who, samples, iters)) return -1;
  if (!current_plane != !current_var) return pt_fail("%s: the current plane and its variance come together or not at all", who);
  return 0;
}
extern "C" int pt_history_noise_host(int pixels, const float* noise_planes, int groups, int64_t iters, float samples, const float* current_plane,
                                     const float* current_var, float* w_out, double* sse) {
  if (pt_history_noise_check("pt_history_noise_host", pixels, noise_planes, groups, iters, samples, current_plane, current_var)) return -1;
  const Fold f = ptnz::fold_scalars(1, groups, iters);
  const double s = pthi::noise_host((size_t)pixels, noise_planes, f.Tf, f.Df, samples, current_plane, current_var, w_out);
  if (sse) *sse = s;
  return 0;
}

extern "C" int pt_noise_fold_host(int pixels, const float* rgb_sum, float* planes, int group_iters, int groups_after, int64_t iters_after,
                                  double* sse) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum || !planes) return pt_fail("pt_noise_fold_host: bad argument");
  if (group_iters < 1 || groups_after < 1 || iters_after < (int64_t)group_iters + (groups_after - 1))
    return pt_fail("pt_noise_fold_host: a group of %d iterations cannot be group %d of %lld iterations (every group holds at least one)", group_iters,
                   groups_after, (long long)iters_after);
  const Fold f = ptnz::fold_scalars(group_iters, groups_after, iters_after);
  const double s = ptnz::fold_host((size_t)pixels, rgb_sum, planes, f);
  if (sse) *sse = groups_after >= 2 ? s : -1.0;
  return 0;
}
