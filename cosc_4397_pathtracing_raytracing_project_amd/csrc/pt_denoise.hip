// pt_denoise.hip — the kernels of the edge-avoiding à-trous filter (include/pt_amd.h pt_denoise) and their launcher.
//
// A translation unit of its own, compiled ONCE with -ffp-contract=off: the filter is specified as separate IEEE float32 operations
// (pt_denoise.h), so there is nothing an arithmetic mode could change, and the path tracer's kernels (pt_kernels.hip) are not
// rebuilt differently because of it.  The kernels are thin: thread indices in, the PT_HD bodies of pt_denoise.h, which the host
// loop pt_denoise_host runs too.
//
//   k_denoise_prepare   one thread per pixel: SUM image + feature SUM planes -> normal | hit, position, albedo, colour (4 x 16 B)
//   k_denoise_level     the hot path, once per level: a 64 x 4 workgroup, lanes along x (at every step consecutive lanes read
//                       consecutive pixels: 1 KiB per wave and load), each thread kRows pixels of its column, rows s apart
//                       (pt_denoise.h level_column); no LDS, the reuse left between neighbouring columns is L1's and L2's
//   k_denoise_finish    one thread per pixel: remodulation, 12 B per pixel
// The variance-guided form (pt_denoise_guided) runs the same mapping with its own bodies and shares k_denoise_finish:
//   k_denoise_prepare_guided   k_denoise_prepare + the two noise planes in, var_raw out in the albedo's spare word
//   k_denoise_var_prefilter    one thread per pixel, 64 x 4 tiles: 3 x 3 over var_raw and the hit flags, var_0 into colour buffer 0's .w
//   k_denoise_level_guided     k_denoise_level's shape and loads (the variance rides in the colour's .w); per centre two more
//                              registers (its colour factor, the sum of w^2 var), per tap a multiply and a multiply-add
// The adaptive form (pt_denoise_adaptive) replaces the first two of those and runs k_denoise_level_guided and k_denoise_finish as they are:
//   k_denoise_prepare_adaptive        k_denoise_prepare_guided with the pixel's own counts (8 B more in; the count plane, or the fold's
//                                     two scalars in the uniform state), Tf_p out in the position's spare word
//   k_denoise_var_prefilter_adaptive  k_denoise_var_prefilter over var_raw * Tf of the nine neighbours (n.w, a.w, p.w), back in the centre's unit
#include <hip/hip_runtime.h>

#include "pt_denoise.h"
#include "pt_internal.h"
#include "pt_noise.h"

namespace {
using ptdn::Params;
using ptdn::V4;
constexpr int kBlock = 256;
constexpr int kLevelX = 64, kLevelY = kBlock / kLevelX;  // a wave is 64 pixels of one row slot

__global__ __launch_bounds__(kBlock) void k_denoise_prepare(int npix, const float* __restrict__ S, const V4* __restrict__ planes, float samples,
                                                            int keep_albedo, V4* __restrict__ n, V4* __restrict__ p, V4* __restrict__ a,
                                                            V4* __restrict__ c) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) ptdn::prepare_pixel((size_t)i, (size_t)npix, S, planes, samples, keep_albedo, n, p, a, c);
}

__global__ __launch_bounds__(kBlock) void k_denoise_level(int W, int R, int l, Params P, const V4* __restrict__ c, const V4* __restrict__ n,
                                                          const V4* __restrict__ p, V4* __restrict__ out) {
  const int x = blockIdx.x * kLevelX + (threadIdx.x & (kLevelX - 1));
  const int ty = blockIdx.y * kLevelY + threadIdx.x / kLevelX;
  if (x < W && ty < ptdn::level_slots(R, l)) ptdn::level_column(W, R, x, ty, l, P, c, n, p, out);
}

__global__ __launch_bounds__(kBlock) void k_denoise_finish(int npix, int keep_albedo, const V4* __restrict__ c, const V4* __restrict__ a,
                                                           float* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) ptdn::finish_pixel((size_t)i, keep_albedo, c, a, out);
}

__global__ __launch_bounds__(kBlock) void k_denoise_prepare_guided(int npix, const float* __restrict__ S, const V4* __restrict__ planes,
                                                                   const V4* __restrict__ noise, float Tf, float Df, int keep_albedo, V4* __restrict__ n,
                                                                   V4* __restrict__ p, V4* __restrict__ a, V4* __restrict__ c) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) ptdn::prepare_pixel_guided((size_t)i, (size_t)npix, S, planes, noise, Tf, Df, keep_albedo, n, p, a, c);
}

__global__ __launch_bounds__(kBlock) void k_denoise_var_prefilter(int W, int R, const V4* __restrict__ n, const V4* __restrict__ a, V4* __restrict__ c0) {
  const int x = blockIdx.x * kLevelX + (threadIdx.x & (kLevelX - 1));
  const int y = blockIdx.y * kLevelY + threadIdx.x / kLevelX;
  if (x < W && y < R) ptdn::var_prefilter_pixel(W, R, x, y, n, a, c0);
}

__global__ __launch_bounds__(kBlock) void k_denoise_level_guided(int W, int R, int l, Params P, const V4* __restrict__ c, const V4* __restrict__ n,
                                                                 const V4* __restrict__ p, V4* __restrict__ out) {
  const int x = blockIdx.x * kLevelX + (threadIdx.x & (kLevelX - 1));
  const int ty = blockIdx.y * kLevelY + threadIdx.x / kLevelX;
  if (x < W && ty < ptdn::level_slots(R, l)) ptdn::level_column_guided(W, R, x, ty, l, P, c, n, p, out);
}

__global__ __launch_bounds__(kBlock) void k_denoise_prepare_adaptive(int npix, const float* __restrict__ S, const V4* __restrict__ planes,
                                                                     const V4* __restrict__ noise, const ptad::Cnt* __restrict__ cnt, int T, int M,
                                                                     int keep_albedo, V4* __restrict__ n, V4* __restrict__ p, V4* __restrict__ a,
                                                                     V4* __restrict__ c) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) ptdn::prepare_pixel_adaptive((size_t)i, (size_t)npix, S, planes, noise, cnt, T, M, keep_albedo, n, p, a, c);
}

__global__ __launch_bounds__(kBlock) void k_denoise_var_prefilter_adaptive(int W, int R, const V4* __restrict__ n, const V4* __restrict__ a,
                                                                           const V4* __restrict__ p, V4* __restrict__ c0) {
  const int x = blockIdx.x * kLevelX + (threadIdx.x & (kLevelX - 1));
  const int y = blockIdx.y * kLevelY + threadIdx.x / kLevelX;
  if (x < W && y < R) ptdn::var_prefilter_pixel_adaptive(W, R, x, y, n, a, p, c0);
}

}  // namespace

// pt_internal.h.  Everything is checked before the first launch; no allocation, no synchronisation.
int pt_denoise_launch(hipStream_t stream, int w, int rows, const float* rgb_sum_dev, const float* planes_dev, float samples,
                      const ptdn::Params& P, void* workspace_dev, const float** rgb_avg_dev) {
  if (w <= 0 || rows <= 0 || rows >= 32768 || (int64_t)w * rows > (1ll << 30)) return pt_fail("pt_denoise: a frame of %d x %d pixels is not supported", w, rows);
  if (!rgb_sum_dev || !planes_dev || !workspace_dev || !(samples > 0.0f) || P.levels < 1 || P.levels > ptdn::kMaxLevels)
    return pt_fail("pt_denoise: bad argument");
  const int npix = w * rows;
  V4* n = static_cast<V4*>(workspace_dev);
  V4 *p = n + npix, *a = p + npix, *col[2] = {a + npix, a + 2 * (size_t)npix};
  const int flat = (npix + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_denoise_prepare, dim3(flat), dim3(kBlock), 0, stream, npix, rgb_sum_dev, reinterpret_cast<const V4*>(planes_dev), samples,
                     P.keep_albedo, n, p, a, col[0]);
  for (int l = 0; l < P.levels; ++l) {
    const dim3 grid((w + kLevelX - 1) / kLevelX, (ptdn::level_slots(rows, l) + kLevelY - 1) / kLevelY);
    hipLaunchKernelGGL(k_denoise_level, grid, dim3(kBlock), 0, stream, w, rows, l, P, col[ptdn::color_buffer(l)], n, p, col[ptdn::color_buffer(l + 1)]);
  }
  float* out = reinterpret_cast<float*>(col[ptdn::color_buffer(P.levels + 1)]);
  hipLaunchKernelGGL(k_denoise_finish, dim3(flat), dim3(kBlock), 0, stream, npix, P.keep_albedo, col[ptdn::color_buffer(P.levels)], a, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pt_fail("pt_denoise: launch failed: %s", hipGetErrorString(e));
  if (rgb_avg_dev) *rgb_avg_dev = out;
  return 0;
}

int pt_denoise_guided_launch(hipStream_t stream, int w, int rows, const float* rgb_sum_dev, const float* planes_dev, const float* noise_dev, float Tf,
                             float Df, const ptdn::Params& P, void* workspace_dev, const float** rgb_avg_dev) {
  if (w <= 0 || rows <= 0 || rows >= 32768 || (int64_t)w * rows > (1ll << 30)) return pt_fail("pt_denoise_guided: a frame of %d x %d pixels is not supported", w, rows);
  if (!rgb_sum_dev || !planes_dev || !noise_dev || !workspace_dev || !(Tf >= 2.0f) || !(Df >= Tf) || P.levels < 1 || P.levels > ptdn::kMaxLevels)
    return pt_fail("pt_denoise_guided: bad argument");
  const int npix = w * rows;
  V4* n = static_cast<V4*>(workspace_dev);
  V4 *p = n + npix, *a = p + npix, *col[2] = {a + npix, a + 2 * (size_t)npix};
  const int flat = (npix + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_denoise_prepare_guided, dim3(flat), dim3(kBlock), 0, stream, npix, rgb_sum_dev, reinterpret_cast<const V4*>(planes_dev),
                     reinterpret_cast<const V4*>(noise_dev), Tf, Df, P.keep_albedo, n, p, a, col[0]);
  hipLaunchKernelGGL(k_denoise_var_prefilter, dim3((w + kLevelX - 1) / kLevelX, (rows + kLevelY - 1) / kLevelY), dim3(kBlock), 0, stream, w, rows, n, a, col[0]);
  for (int l = 0; l < P.levels; ++l) {
    const dim3 grid((w + kLevelX - 1) / kLevelX, (ptdn::level_slots(rows, l) + kLevelY - 1) / kLevelY);
    hipLaunchKernelGGL(k_denoise_level_guided, grid, dim3(kBlock), 0, stream, w, rows, l, P, col[ptdn::color_buffer(l)], n, p, col[ptdn::color_buffer(l + 1)]);
  }
  float* out = reinterpret_cast<float*>(col[ptdn::color_buffer(P.levels + 1)]);
  hipLaunchKernelGGL(k_denoise_finish, dim3(flat), dim3(kBlock), 0, stream, npix, P.keep_albedo, col[ptdn::color_buffer(P.levels)], a, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pt_fail("pt_denoise_guided: launch failed: %s", hipGetErrorString(e));
  if (rgb_avg_dev) *rgb_avg_dev = out;
  return 0;
}

int pt_denoise_adaptive_launch(hipStream_t stream, int w, int rows, const float* rgb_sum_dev, const float* planes_dev, const float* noise_dev,
                               const void* counts_dev, int iters, int groups, const ptdn::Params& P, void* workspace_dev, const float** rgb_avg_dev) {
  if (w <= 0 || rows <= 0 || rows >= 32768 || (int64_t)w * rows > (1ll << 30)) return pt_fail("pt_denoise_adaptive: a frame of %d x %d pixels is not supported", w, rows);
  if (!rgb_sum_dev || !planes_dev || !noise_dev || !workspace_dev || (!counts_dev && (groups < 2 || iters < groups)) || P.levels < 1 || P.levels > ptdn::kMaxLevels)
    return pt_fail("pt_denoise_adaptive: bad argument");
  const int npix = w * rows;
  V4* n = static_cast<V4*>(workspace_dev);
  V4 *p = n + npix, *a = p + npix, *col[2] = {a + npix, a + 2 * (size_t)npix};
  const int flat = (npix + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_denoise_prepare_adaptive, dim3(flat), dim3(kBlock), 0, stream, npix, rgb_sum_dev, reinterpret_cast<const V4*>(planes_dev),
                     reinterpret_cast<const V4*>(noise_dev), static_cast<const ptad::Cnt*>(counts_dev), iters, groups, P.keep_albedo, n, p, a, col[0]);
  hipLaunchKernelGGL(k_denoise_var_prefilter_adaptive, dim3((w + kLevelX - 1) / kLevelX, (rows + kLevelY - 1) / kLevelY), dim3(kBlock), 0, stream, w, rows, n,
                     a, p, col[0]);
  for (int l = 0; l < P.levels; ++l) {
    const dim3 grid((w + kLevelX - 1) / kLevelX, (ptdn::level_slots(rows, l) + kLevelY - 1) / kLevelY);
    hipLaunchKernelGGL(k_denoise_level_guided, grid, dim3(kBlock), 0, stream, w, rows, l, P, col[ptdn::color_buffer(l)], n, p, col[ptdn::color_buffer(l + 1)]);
  }
  float* out = reinterpret_cast<float*>(col[ptdn::color_buffer(P.levels + 1)]);
  hipLaunchKernelGGL(k_denoise_finish, dim3(flat), dim3(kBlock), 0, stream, npix, P.keep_albedo, col[ptdn::color_buffer(P.levels)], a, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pt_fail("pt_denoise_adaptive: launch failed: %s", hipGetErrorString(e));
  if (rgb_avg_dev) *rgb_avg_dev = out;
  return 0;
}

int pt_denoise_resolve(const char* who, float samples, const PtDenoiseOptions* opt, ptdn::Params* P) {
  if (!(samples > 0.0f)) return pt_fail("%s: samples must be positive", who);
  if (const char* msg = ptdn::resolve(opt, P)) return pt_fail("%s: %s", who, msg);
  return 0;
}

extern "C" int pt_denoise_host(int w, int rows, const float* rgb_sum, const float* planes, float samples, const PtDenoiseOptions* opt, float* rgb_avg) {
  if (w <= 0 || rows <= 0 || (int64_t)w * rows > (1ll << 30) || !rgb_sum || !planes || !rgb_avg) return pt_fail("pt_denoise_host: bad argument");
  ptdn::Params P{};
  if (pt_denoise_resolve("pt_denoise_host", samples, opt, &P)) return -1;
  ptdn::denoise_host(w, rows, rgb_sum, planes, samples, P, rgb_avg);
  return 0;
}

int pt_denoise_guided_resolve(const char* who, int groups, int64_t iters, const PtDenoiseOptions* opt, ptdn::Params* P, float* Tf, float* Df) {
  if (groups < 2) return pt_fail("%s: %d group(s) folded; a variance needs at least 2 (pt_noise_fold after each group of iterations)", who, groups);
  if (iters < groups) return pt_fail("%s: %d groups cannot hold %lld iterations (every group holds at least one)", who, groups, (long long)iters);
  if (const char* msg = ptdn::resolve(opt, P, ptdn::kGuidedSigmaColor)) return pt_fail("%s: %s", who, msg);
  const ptnz::Fold f = ptnz::fold_scalars(1, groups, iters);
  *Tf = f.Tf, *Df = f.Df;
  return 0;
}

namespace {
int guided_host(const char* who, int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups, int64_t iters,
                const PtDenoiseOptions* opt, float* rgb_avg, float* var_raw, float* var_0) {
  if (w <= 0 || rows <= 0 || (int64_t)w * rows > (1ll << 30) || !rgb_sum || !planes || !noise_planes) return pt_fail("%s: bad argument", who);
  ptdn::Params P{};
  float Tf = 0.0f, Df = 0.0f;
  if (pt_denoise_guided_resolve(who, groups, iters, opt, &P, &Tf, &Df)) return -1;
  ptdn::denoise_guided_host(w, rows, rgb_sum, planes, noise_planes, Tf, Df, P, rgb_avg, var_raw, var_0);
  return 0;
}
}  // namespace

extern "C" int pt_denoise_guided_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups, int64_t iters,
                                      const PtDenoiseOptions* opt, float* rgb_avg) {
  if (!rgb_avg) return pt_fail("pt_denoise_guided_host: bad argument");
  return guided_host("pt_denoise_guided_host", w, rows, rgb_sum, planes, noise_planes, groups, iters, opt, rgb_avg, nullptr, nullptr);
}

extern "C" int pt_denoise_guided_variance_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups,
                                               int64_t iters, const PtDenoiseOptions* opt, float* var_raw, float* var_0) {
  return guided_host("pt_denoise_guided_variance_host", w, rows, rgb_sum, planes, noise_planes, groups, iters, opt, nullptr, var_raw, var_0);
}

int pt_denoise_adaptive_resolve(const char* who, const PtDenoiseOptions* opt, ptdn::Params* P) {
  if (const char* msg = ptdn::resolve(opt, P, ptdn::kGuidedSigmaColor)) return pt_fail("%s: %s", who, msg);
  return 0;
}

int pt_denoise_adaptive_check(const char* who, int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                              const PtDenoiseOptions* opt, ptdn::Params* P) {
  if (w <= 0 || rows <= 0 || (int64_t)w * rows > (1ll << 30)) return pt_fail("%s: a frame of %d x %d pixels is not supported", who, w, rows);
  if (!rgb_sum || !planes || !noise_planes || !counts) return pt_fail("%s: null argument", who);
  const size_t npix = (size_t)w * rows;
  for (size_t i = 0; i < npix; ++i)
    if (counts[2 * i + 1] < 2 || counts[2 * i] < counts[2 * i + 1])
      return pt_fail("%s: pixel %zu has T = %d iterations in M = %d groups; a variance needs M >= 2 and T >= M", who, i, counts[2 * i], counts[2 * i + 1]);
  return pt_denoise_adaptive_resolve(who, opt, P);
}

extern "C" int pt_denoise_adaptive_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                                        const PtDenoiseOptions* opt, float* rgb_avg) {
  if (!rgb_avg) return pt_fail("pt_denoise_adaptive_host: null argument");
  ptdn::Params P{};
  if (pt_denoise_adaptive_check("pt_denoise_adaptive_host", w, rows, rgb_sum, planes, noise_planes, counts, opt, &P)) return -1;
  ptdn::denoise_adaptive_host(w, rows, rgb_sum, planes, noise_planes, counts, P, rgb_avg);
  return 0;
}

extern "C" int pt_denoise_adaptive_variance_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes,
                                                 const int32_t* counts, const PtDenoiseOptions* opt, float* var_raw, float* var_0) {
  ptdn::Params P{};
  if (pt_denoise_adaptive_check("pt_denoise_adaptive_variance_host", w, rows, rgb_sum, planes, noise_planes, counts, opt, &P)) return -1;
  ptdn::denoise_adaptive_host(w, rows, rgb_sum, planes, noise_planes, counts, P, nullptr, var_raw, var_0);
  return 0;
}
