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
#include <hip/hip_runtime.h>

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
