// pt_history_threshold.hip — threshold rounds over the blend (include/pt_amd.h pt_history_round_threshold): the history steps that read
// per-pixel sample counts, their launchers and their host twins.
//
// A translation unit of its own, compiled ONCE with -ffp-contract=off like pt_history.hip and pt_noise.hip, so that the kernels of
// those files are the code they were.  The arithmetic is pt_history.h's PT_HD bodies (Counts, noise_counts_pixel, key_blend_pixel,
// blend_counts_pixel, capture_counts_pixel), which the host loops run too.  One thread per tile pixel in workgroups of 256, consecutive
// lanes on consecutive pixels, 16-byte plane accesses, the last workgroup ragged; cnt (8 B per pixel) is read only in the adaptive
// state — in the uniform state the fold's (T, M) arrive as two scalars.
//
//   k_history_noise_counts   pass A, k_history_noise's shape (a workgroup owns PT_NOISE_PIXELS_PER_PARTIAL pixels): 32 B of the fold's
//                            planes, 8 B of cnt and (C, VC present) the .w word of C and 16 B of VC in; 4 B of W and 4 B of NE out per
//                            pixel, one double per workgroup from the fold's tree (LDS: the four wave sums), no atomics
//   k_history_key_blend      pass B: 9 taps of W and of NE through L1 (k_adaptive_key's pattern), 4 B of key out
//   k_history_blend_counts   streaming: 12 B of S, 8 B of cnt and (when present) 16 B of C in, 12 B out per pixel
//   k_history_capture_counts streaming: 12 B of S, 48 B of feature sums, 32 B of the fold's planes, 8 B of cnt and (when present) 16 B of C
//                            and 16 B of VC in, 48 B of K and 16 B of VK out per pixel
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "pt_history.h"
#include "pt_internal.h"
#include "pt_noise.h"

namespace {
using pthi::Counts;
using pthi::V4;
using N4 = ptnz::V4;
constexpr int kBlock = 256;
constexpr int kPerThread = PT_NOISE_PIXELS_PER_PARTIAL / kBlock;
constexpr int kWaves = kBlock / 64;
static_assert(kPerThread * kBlock == PT_NOISE_PIXELS_PER_PARTIAL && kBlock % 64 == 0, "a workgroup owns exactly one partial sum");

__global__ __launch_bounds__(kBlock) void k_history_noise_counts(int npix, const N4* __restrict__ planes, Counts cnt, const V4* __restrict__ C,
                                                                 const V4* __restrict__ VC, float* __restrict__ W, float* __restrict__ NE,
                                                                 double* __restrict__ partial) {
  __shared__ double wave_sum[kWaves];
  const size_t base = (size_t)blockIdx.x * PT_NOISE_PIXELS_PER_PARTIAL + threadIdx.x;
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const size_t i = base + (size_t)j * kBlock;
    if (i < (size_t)npix) sum += (double)pthi::noise_counts_pixel(i, (size_t)npix, planes, cnt, C, VC, W, NE, static_cast<V4*>(nullptr));
  }
  // k_noise_fold's tree: shuffles inside a wave, then the four waves in order
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = wave_sum[0];
    for (int w = 1; w < kWaves; ++w) s += wave_sum[w];
    partial[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kBlock) void k_history_key_blend(int W, int R, const float* __restrict__ Wp, const float* __restrict__ NE,
                                                              uint32_t* __restrict__ key) {
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= (size_t)W * R) return;
  const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
  key[p] = pthi::key_blend_pixel(x, y, W, R, Wp, NE);
}

__global__ __launch_bounds__(kBlock) void k_history_blend_counts(int npix, const float* __restrict__ S, Counts cnt, const V4* __restrict__ C,
                                                                 float* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) pthi::blend_counts_pixel((size_t)i, S, cnt, C, out);
}

__global__ __launch_bounds__(kBlock) void k_history_capture_counts(int npix, const float* __restrict__ S, const V4* __restrict__ feat,
                                                                   const N4* __restrict__ planes, Counts cnt, const V4* C, const V4* VC, V4* __restrict__ K,
                                                                   V4* __restrict__ VK) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) pthi::capture_counts_pixel((size_t)i, (size_t)npix, S, feat, planes, cnt, C, VC, K, VK);
}

int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : pt_fail("%s: launch failed: %s", who, hipGetErrorString(e));
}
// counts_dev, or the fold's (T, M) for every pixel; M >= 2 and T >= M either way (the plane's entries: the callers' business)
bool bad_counts(const void* counts_dev, int iters, int groups) { return !counts_dev && (groups < 2 || iters < groups); }
Counts counts_of(const void* counts_dev, int iters, int groups) { return Counts{static_cast<const ptad::Cnt*>(counts_dev), iters, groups}; }
unsigned blocks_of(int n) { return (unsigned)((n + kBlock - 1) / kBlock); }
}  // namespace

// pt_internal.h.  Everything is checked before the launch; no allocation, no synchronisation.
int pt_history_noise_counts_launch(hipStream_t stream, int pixels, const void* state_dev, const void* counts_dev, int iters, int groups, const void* current_dev,
                                   const void* current_var_dev, void* out_dev, float* ne_dev, bool reduce) {
  if (pixels <= 0 || pixels > (1 << 30) || !state_dev || bad_counts(counts_dev, iters, groups) || !current_dev != !current_var_dev || !out_dev || !ne_dev)
    return pt_fail("pt_history_noise_adaptive: bad argument");
  const int blocks = (int)pt_noise_partials((size_t)pixels);
  double* partial = static_cast<double*>(out_dev);
  hipLaunchKernelGGL(k_history_noise_counts, dim3(blocks), dim3(kBlock), 0, stream, pixels, static_cast<const N4*>(state_dev), counts_of(counts_dev, iters, groups),
                     static_cast<const V4*>(current_dev), static_cast<const V4*>(current_var_dev), pt_history_noise_plane(out_dev, (size_t)pixels), ne_dev, partial);
  if (launched("pt_history_noise_adaptive")) return -1;
  return reduce ? pt_noise_reduce_launch(stream, blocks, partial, partial + blocks) : 0;
}
int pt_history_key_blend_launch(hipStream_t stream, int w, int rows, const float* w_dev, const float* ne_dev, uint32_t* key_dev) {
  if (w <= 0 || rows <= 0 || rows >= 32768 || (int64_t)w * rows > (1ll << 30) || !w_dev || !ne_dev || !key_dev)
    return pt_fail("pt_history_round_threshold: bad argument");
  hipLaunchKernelGGL(k_history_key_blend, dim3(blocks_of(w * rows)), dim3(kBlock), 0, stream, w, rows, w_dev, ne_dev, key_dev);
  return launched("pt_history_round_threshold");
}
int pt_history_blend_counts_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const void* counts_dev, int iters, int groups,
                                   const void* current_dev, float* rgb_avg_dev) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum_dev || !rgb_avg_dev || bad_counts(counts_dev, iters, groups))
    return pt_fail("pt_history_resolve_adaptive: bad argument");
  hipLaunchKernelGGL(k_history_blend_counts, dim3(blocks_of(pixels)), dim3(kBlock), 0, stream, pixels, rgb_sum_dev, counts_of(counts_dev, iters, groups),
                     static_cast<const V4*>(current_dev), rgb_avg_dev);
  return launched("pt_history_resolve_adaptive");
}
int pt_history_capture_counts_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const float* planes_dev, const void* state_dev,
                                     const void* counts_dev, int iters, int groups, const void* current_dev, const void* current_var_dev, void* kept_dev,
                                     void* kept_var_dev) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum_dev || !planes_dev || !state_dev || bad_counts(counts_dev, iters, groups) || !kept_dev || !kept_var_dev ||
      !current_dev != !current_var_dev)
    return pt_fail("pt_history_capture_adaptive: bad argument");
  hipLaunchKernelGGL(k_history_capture_counts, dim3(blocks_of(pixels)), dim3(kBlock), 0, stream, pixels, rgb_sum_dev, reinterpret_cast<const V4*>(planes_dev),
                     static_cast<const N4*>(state_dev), counts_of(counts_dev, iters, groups), static_cast<const V4*>(current_dev),
                     static_cast<const V4*>(current_var_dev), static_cast<V4*>(kept_dev), static_cast<V4*>(kept_var_dev));
  return launched("pt_history_capture_adaptive");
}

// What the host and stage forms refuse in their counts: the first pixel with M_p < 2 or T_p < M_p is named (pt_denoise_adaptive_host's
// words), then a current plane without its variance.
int pt_history_counts_check(const char* who, int pixels, const int32_t* counts, const float* current_plane, const float* current_var) {
  if (!counts) return pt_fail("%s: bad argument", who);
  for (int p = 0; p < pixels; ++p)
    if (counts[2 * (size_t)p + 1] < 2 || counts[2 * (size_t)p] < counts[2 * (size_t)p + 1])
      return pt_fail("%s: pixel %d has T_p = %d iterations in M_p = %d groups; a variance needs M_p >= 2 and T_p >= M_p", who, p, counts[2 * (size_t)p],
                     counts[2 * (size_t)p + 1]);
  if (!current_plane != !current_var) return pt_fail("%s: the current plane and its variance come together or not at all", who);
  return 0;
}

extern "C" int pt_history_noise_adaptive_host(int pixels, const float* noise_planes, const int32_t* counts, const float* current_plane, const float* current_var,
                                              float* w_out, float* ne_out, float* vb_out, double* sse) {
  const char* who = "pt_history_noise_adaptive_host";
  if (pixels <= 0 || pixels > (1 << 30) || !noise_planes) return pt_fail("%s: bad argument", who);
  if (pt_history_counts_check(who, pixels, counts, current_plane, current_var)) return -1;
  std::vector<float> w, ne;  // W and NE are what the loop writes; a caller may want neither
  if (!w_out) w.resize((size_t)pixels), w_out = w.data();
  if (!ne_out) ne.resize((size_t)pixels), ne_out = ne.data();
  const double s = pthi::noise_counts_host((size_t)pixels, noise_planes, counts, current_plane, current_var, w_out, ne_out, vb_out);
  if (sse) *sse = s;
  return 0;
}

extern "C" int pt_history_select_threshold_blend_host(int w, int rows, const float* noise_planes, const int32_t* counts, const float* current_plane,
                                                      const float* current_var, float threshold, int cap, int32_t* list, int* above, int* m) {
  const char* who = "pt_history_select_threshold_blend_host";
  if (pt_adaptive_check_select(who, w, rows, noise_planes, counts, cap, list)) return -1;
  if (pt_adaptive_check_threshold(who, threshold)) return -1;
  if (!above || !m) return pt_fail("%s: bad argument", who);
  if (pt_history_counts_check(who, w * rows, counts, current_plane, current_var)) return -1;
  pthi::select_threshold_blend_host(w, rows, noise_planes, counts, current_plane, current_var, threshold, cap, list, above, m);
  return 0;
}

extern "C" int pt_history_blend_adaptive_host(int pixels, const float* rgb_sum, const int32_t* counts, const float* current_plane, float* rgb_avg) {
  const char* who = "pt_history_blend_adaptive_host";
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum || !rgb_avg) return pt_fail("%s: bad argument", who);
  if (pt_history_counts_check(who, pixels, counts, nullptr, nullptr)) return -1;
  pthi::blend_counts_host((size_t)pixels, rgb_sum, counts, current_plane, rgb_avg);
  return 0;
}

extern "C" int pt_history_capture_adaptive_host(int pixels, const float* rgb_sum, const float* feature_planes, const float* noise_planes, const int32_t* counts,
                                                const float* current_plane, const float* current_var, float* kept_planes, float* kept_var) {
  const char* who = "pt_history_capture_adaptive_host";
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum || !feature_planes || !noise_planes || !kept_planes || !kept_var) return pt_fail("%s: bad argument", who);
  if (pt_history_counts_check(who, pixels, counts, current_plane, current_var)) return -1;
  pthi::capture_counts_host((size_t)pixels, rgb_sum, feature_planes, noise_planes, counts, current_plane, current_var, kept_planes, kept_var);
  return 0;
}
