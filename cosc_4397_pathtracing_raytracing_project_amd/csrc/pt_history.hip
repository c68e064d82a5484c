// pt_history.hip — the kernels of the reprojected sample history (include/pt_amd.h pt_history_capture) and their launchers.
//
// A translation unit of its own, compiled ONCE with -ffp-contract=off like pt_denoise.hip and pt_noise.hip: the history is specified
// as separate IEEE float32 operations (pt_history.h), so there is nothing an arithmetic mode could change, and the path tracer's
// kernels (pt_kernels.hip) are not touched.  The kernels are thin: one thread per tile pixel, the PT_HD bodies of pt_history.h,
// which the host loops run too; consecutive lanes own consecutive pixels, every plane access is 16 bytes per lane (1 KiB per wave),
// the last workgroup is ragged.
//
//   k_history_capture    streaming: 12 B of S, 48 B of feature sums and (when present) 16 B of C in, 48 B of K out per pixel
//   k_history_reproject  a gather: 48 B of feature sums in and 16 B of C out per pixel, streaming; per tap of the 2 x 2 footprint
//                        16 B of K1, then 16 B of K2, then — for a tap that passed — 16 B of K0.  Neighbouring pixels of the new
//                        view land on neighbouring pixels of the kept one, so the taps of a wave are a few runs of rows of K and
//                        the four taps of a pixel share lines with its neighbours': the reuse is L1's and L2's, no LDS
//   k_history_blend      streaming: 12 B of S and (when present) 16 B of C in, 12 B out per pixel
#include <hip/hip_runtime.h>

#include "pt_history.h"
#include "pt_internal.h"

namespace {
using pthi::Params;
using pthi::V4;
using pthi::View;
constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_history_capture(int npix, const float* __restrict__ S, const V4* __restrict__ feat, const V4* C, float samples,
                                                            V4* __restrict__ K) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) pthi::capture_pixel((size_t)i, (size_t)npix, S, feat, C, samples, K);
}

__global__ __launch_bounds__(kBlock) void k_history_reproject(int npix, View v, const V4* __restrict__ K, const V4* __restrict__ feat,
                                                              const uint8_t* __restrict__ reject, int num_geoms, Params P, V4* __restrict__ C) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) C[i] = pthi::reproject_pixel((size_t)i, v, K, feat, reject, num_geoms, P);
}

__global__ __launch_bounds__(kBlock) void k_history_blend(int npix, const float* __restrict__ S, float samples, const V4* __restrict__ C,
                                                          float* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) pthi::blend_pixel((size_t)i, S, samples, C, out);
}

int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pt_fail("%s: launch failed: %s", who, hipGetErrorString(e));
  return 0;
}
bool bad_frame(int w, int rows) { return w <= 0 || rows <= 0 || rows >= 32768 || (int64_t)w * rows > (1ll << 30); }
}  // namespace

// pt_internal.h.  Everything is checked before the launch; no allocation, no synchronisation.
int pt_history_capture_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const float* planes_dev, const void* current_dev, float samples,
                              void* kept_dev) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum_dev || !planes_dev || !kept_dev || !(samples > 0.0f)) return pt_fail("pt_history_capture: bad argument");
  hipLaunchKernelGGL(k_history_capture, dim3((pixels + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pixels, rgb_sum_dev,
                     reinterpret_cast<const V4*>(planes_dev), static_cast<const V4*>(current_dev), samples, static_cast<V4*>(kept_dev));
  return launched("pt_history_capture");
}

int pt_history_reproject_launch(hipStream_t stream, const pthi::View& v, const void* kept_dev, const float* planes_dev, const uint8_t* reject_dev,
                                int num_geoms, const pthi::Params& P, void* current_dev) {
  if (bad_frame(v.W, v.R)) return pt_fail("pt_history_reproject: a tile of %d x %d pixels is not supported", v.W, v.R);
  if (!kept_dev || !planes_dev || !current_dev || (!P.keep_view_dependent && (num_geoms < 0 || (num_geoms > 0 && !reject_dev))))
    return pt_fail("pt_history_reproject: bad argument");
  const int npix = v.W * v.R;
  hipLaunchKernelGGL(k_history_reproject, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, npix, v, static_cast<const V4*>(kept_dev),
                     reinterpret_cast<const V4*>(planes_dev), reject_dev, num_geoms, P, static_cast<V4*>(current_dev));
  return launched("pt_history_reproject");
}

int pt_history_blend_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, float samples, const void* current_dev, float* rgb_avg_dev) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum_dev || !rgb_avg_dev || !(samples > 0.0f)) return pt_fail("pt_history_resolve: bad argument");
  hipLaunchKernelGGL(k_history_blend, dim3((pixels + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pixels, rgb_sum_dev, samples,
                     static_cast<const V4*>(current_dev), rgb_avg_dev);
  return launched("pt_history_resolve");
}

int pt_history_check_samples(const char* who, float samples) {
  if (!(samples - samples == 0.0f) || !(samples > 0.0f)) return pt_fail("%s: samples must be finite and positive", who);
  return 0;
}
int pt_history_resolve_options(const char* who, const PtHistoryOptions* opt, pthi::Params* P) {
  if (const char* msg = pthi::resolve(opt, P)) return pt_fail("%s: %s", who, msg);
  return 0;
}
// What the host and stage forms of the reprojection refuse: the frame, the arrays, a kept camera of another width, then the options.
int pt_history_reproject_check(const char* who, int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                               const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* current_plane, pthi::Params* P) {
  if (w <= 0 || rows <= 0 || (int64_t)w * rows > (1ll << 30)) return pt_fail("%s: a tile of %d x %d pixels is not supported", who, w, rows);
  if (!kept_cam || !kept_planes || !feature_planes || !current_plane) return pt_fail("%s: null argument", who);
  if (kept_cam->resolution[0] != w || row0 < 0 || (int64_t)row0 + rows > kept_cam->resolution[1])
    return pt_fail("%s: rows %d .. %d of width %d do not lie in the kept camera's %d x %d frame", who, row0, row0 + rows - 1, w, kept_cam->resolution[0],
                   kept_cam->resolution[1]);
  if (pt_history_resolve_options(who, opt, P)) return -1;
  if (!P->keep_view_dependent && (num_geoms < 0 || (num_geoms > 0 && !reject_geom))) return pt_fail("%s: null reject_geom for %d geoms", who, num_geoms);
  return 0;
}

extern "C" int pt_history_capture_host(int pixels, const float* rgb_sum, const float* feature_planes, const float* current_plane, float samples,
                                       float* kept_planes) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum || !feature_planes || !kept_planes) return pt_fail("pt_history_capture_host: bad argument");
  if (pt_history_check_samples("pt_history_capture_host", samples)) return -1;
  pthi::capture_host((size_t)pixels, rgb_sum, feature_planes, current_plane, samples, kept_planes);
  return 0;
}

extern "C" int pt_history_reproject_host(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                         const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, float* current_plane) {
  pthi::Params P{};
  if (pt_history_reproject_check("pt_history_reproject_host", w, rows, row0, kept_cam, kept_planes, feature_planes, reject_geom, num_geoms, opt, current_plane, &P))
    return -1;
  pthi::reproject_host(pthi::make_view(*kept_cam, rows, row0), kept_planes, feature_planes, reject_geom, num_geoms, P, current_plane);
  return 0;
}

extern "C" int pt_history_blend_host(int pixels, const float* rgb_sum, float samples, const float* current_plane, float* rgb_avg) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum || !rgb_avg) return pt_fail("pt_history_blend_host: bad argument");
  if (pt_history_check_samples("pt_history_blend_host", samples)) return -1;
  pthi::blend_host((size_t)pixels, rgb_sum, samples, current_plane, rgb_avg);
  return 0;
}
