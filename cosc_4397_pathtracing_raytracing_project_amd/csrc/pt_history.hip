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
// What travels beside the history (PT_HISTORY_VARIANCE, PT_HISTORY_MOMENTS) is a template parameter of the first two; <kPlain> and
// <kVariance> are the kernels as they stood before, with the arguments they took, and what flags == 0 launches.
//   k_history_capture<kVariance>  + 32 B of the fold's planes and (when present) 16 B of VC in, 16 B of VK out per pixel
//   k_history_capture<kMoments>   + (when present) 16 B of VC in, 16 B of VK out per pixel; no fold is read
//   k_history_reproject<kVariance>  + 16 B of VC out per pixel; per tap that passed 16 B of VK, read after K0 at the same index
//   k_history_reproject<kMoments>   the same loads and stores; the fourth component of VK is interpolated too
//   k_history_reproject_motion<kPlain | kVariance | kMoments>  the lookup with PT_HISTORY_MOTION: the loads and stores of the kernel
//                        above, one kind byte per pixel and 84 B of a table row for a pixel of a moved geom; launched only when a geom moved
//   k_history_reproject_feedback<bool kMotion>  the moments lookup with PT_HISTORY_FEEDBACK: + 16 B of FC out per pixel; per tap that passed
//                        16 B of FK, read after VK at the same index; <true>: with the motion table, as k_history_reproject_motion.  Kernels
//                        of their own: the ones above are the code they were
// The history round (pt_history_round):
//   k_history_key        a pure stream, one thread per tile pixel: the .w words of the feature sums s1 and s2 and (when present) of C
//                        in, as 4-byte loads 16 bytes apart — 12 B per pixel asked for, whole lines moved: consecutive lanes sit in
//                        the same 128-byte lines, so the planes' 48 B per pixel cross the memory bus as with 16-byte loads, but a lane
//                        holds 3 registers of them, not 12 — one byte of the emitter table for a hit (a gather into a few lines), 4 B
//                        of key out.  No LDS, no scratch
//   k_history_merge      a short scatter, one thread per list entry: 4 B of the list and 12 B of Sw in (streaming), 12 B of S and
//                        4 B of E read and written at the listed pixel
//   k_history_capture_counted<kPlain | kMoments>, k_history_blend_counted   the kernels above with 4 B of E more per pixel in and
//                        ns = samples + E_p for `samples` (pthi::Counted); launched only while E is present
// The history probes (pt_history_probe_keep / _check), P probes of a tile of W x R:
//   k_history_probe_keep      one thread per probe: 12 B of S and the .w words of s1 and s2 at every third pixel of every third row
//                             (a gather: one pixel of three per line moved), 16 B of PK out, streaming
//   k_history_probe_list      one thread per probe: 4 B of the rounds' list out
//   k_history_probe_gradient  one thread per probe: 16 B of PK and 12 B of Sw in (streaming), the same two feature words, one byte of
//                             `moved` for a hit, 4 B of L out; one integer atomic per wave and count (the compiler's wave reduction)
//   k_history_probe_apply     one thread per tile pixel: the .w words of s1 and s2 as k_history_key reads them, one byte of `moved`,
//                             up to (2 radius + 1)^2 words of L (4 B per probe: a ninth of a word per pixel, L1's and L2's), and
//                             C.w read and written in place where the maximum is above 0.  No LDS, no scratch
#include <hip/hip_runtime.h>

#include <type_traits>
#include <vector>

#include "pt_history.h"
#include "pt_internal.h"
#include "pt_noise.h"

namespace {
using pthi::Params;
using pthi::V4;
using pthi::View;
constexpr int kBlock = 256;

// In...: nothing, or the members of pthi::VarCapture (kMoments: pthi::MomCapture) one by one (scalars at fixed offsets; the kPlain
// kernel takes what it took)
template <int kKind, typename... In>
__global__ __launch_bounds__(kBlock) void k_history_capture(int npix, const float* __restrict__ S, const V4* __restrict__ feat, const V4* C, float samples,
                                                            V4* __restrict__ K, In... in) {
  using Side = std::conditional_t<kKind == pthi::kMoments, pthi::MomCapture<V4>, pthi::VarCapture<V4>>;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) pthi::capture_pixel_of<kKind>((size_t)i, (size_t)npix, S, feat, C, samples, K, Side{in...});
}

// In...: nothing, or VK and VC
template <int kKind, typename... In>
__global__ __launch_bounds__(kBlock) void k_history_reproject(int npix, View v, const V4* __restrict__ K, const V4* __restrict__ feat,
                                                              const uint8_t* __restrict__ reject, int num_geoms, Params P, V4* __restrict__ C, In... in) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= npix) return;
  if constexpr (kKind != pthi::kPlain) {
    const auto [VK, VC] = pthi::VarReproject<V4>{in...};
    V4 vh;
    C[i] = pthi::reproject_pixel_of<kKind>((size_t)i, v, K, feat, reject, num_geoms, P, VK, vh);
    VC[i] = vh;
  } else {
    C[i] = pthi::reproject_pixel((size_t)i, v, K, feat, reject, num_geoms, P);
  }
}

// ... with the objects' motion (PT_HISTORY_MOTION): a kernel of its own, so that the ones above are the code they were.  Per pixel
// one byte of `mkind` for a hit that passed the first rejections and, for a moved geom, 84 B of its table row (a few rows per
// frame: they stay in the caches); 11 multiply-adds, a square root and three divisions more.  In...: nothing, or VK and VC
template <int kKind, typename... In>
__global__ __launch_bounds__(kBlock) void k_history_reproject_motion(int npix, View v, const V4* __restrict__ K, const V4* __restrict__ feat,
                                                                     const uint8_t* __restrict__ reject, int num_geoms, Params P,
                                                                     const float* __restrict__ table, const uint8_t* __restrict__ mkind,
                                                                     V4* __restrict__ C, In... in) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= npix) return;
  const pthi::Motion mo{table, mkind};
  V4 vh;
  if constexpr (kKind != pthi::kPlain) {
    const auto [VK, VC] = pthi::VarReproject<V4>{in...};
    C[i] = pthi::reproject_pixel_of<kKind, true>((size_t)i, v, K, feat, reject, num_geoms, P, VK, vh, mo);
    VC[i] = vh;
  } else {
    C[i] = pthi::reproject_pixel_of<kKind, true>((size_t)i, v, K, feat, reject, num_geoms, P, static_cast<const V4*>(nullptr), vh, mo);
  }
}

// ... with the materials' edits (PT_HISTORY_MATERIALS): kernels of their own again.  Per pixel one byte of `rkind` for a hit and, for a
// recoloured geom, the 16 B of its row of `recolor` (one load; a few rows per frame: they stay in the caches); three multiplies more,
// nine with a variance or moments side.  table, mkind: read for kMotion only.  In...: nothing, or VK and VC
template <int kKind, bool kMotion, typename... In>
__global__ __launch_bounds__(kBlock) void k_history_reproject_materials(int npix, View v, const V4* __restrict__ K, const V4* __restrict__ feat,
                                                                        const uint8_t* __restrict__ reject, int num_geoms, Params P,
                                                                        const float* __restrict__ table, const uint8_t* __restrict__ mkind,
                                                                        const float* __restrict__ recolor, const uint8_t* __restrict__ rkind,
                                                                        V4* __restrict__ C, In... in) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= npix) return;
  const pthi::Motion mo{table, mkind};
  const pthi::Recolor rc{recolor, rkind};
  V4 vh;
  if constexpr (kKind != pthi::kPlain) {
    const auto [VK, VC] = pthi::VarReproject<V4>{in...};
    C[i] = pthi::reproject_pixel_materials<kKind, kMotion>((size_t)i, v, K, feat, reject, num_geoms, P, VK, vh, mo, rc);
    VC[i] = vh;
  } else {
    C[i] = pthi::reproject_pixel_materials<kKind, kMotion>((size_t)i, v, K, feat, reject, num_geoms, P, static_cast<const V4*>(nullptr), vh, mo, rc);
  }
}

// ... with the filtered colour beside the moments (PT_HISTORY_FEEDBACK): C and VC are the bits the kernels above write.  table, mkind:
// read for kMotion only.
template <bool kMotion>
__global__ __launch_bounds__(kBlock) void k_history_reproject_feedback(int npix, View v, const V4* __restrict__ K, const V4* __restrict__ feat,
                                                                       const uint8_t* __restrict__ reject, int num_geoms, Params P,
                                                                       const float* __restrict__ table, const uint8_t* __restrict__ mkind,
                                                                       V4* __restrict__ C, const V4* __restrict__ VK, V4* __restrict__ VC,
                                                                       const V4* __restrict__ FK, V4* __restrict__ FC) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= npix) return;
  V4 vh, fc;
  C[i] = pthi::reproject_pixel_of<pthi::kMoments, kMotion, true>((size_t)i, v, K, feat, reject, num_geoms, P, VK, vh, pthi::Motion{table, mkind}, FK, &fc);
  VC[i] = vh;
  FC[i] = fc;
}

__global__ __launch_bounds__(kBlock) void k_history_blend(int npix, const float* __restrict__ S, float samples, const V4* __restrict__ C,
                                                          float* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) pthi::blend_pixel((size_t)i, S, samples, C, out);
}

// ... with the pixel's extras: ns = samples + E[i]
template <int kKind, typename... In>
__global__ __launch_bounds__(kBlock) void k_history_capture_counted(int npix, const float* __restrict__ S, const V4* __restrict__ feat, const V4* C, float samples,
                                                                    const float* __restrict__ E, V4* __restrict__ K, In... in) {
  using Side = std::conditional_t<kKind == pthi::kMoments, pthi::MomCapture<V4>, pthi::VarCapture<V4>>;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) pthi::capture_pixel_of<kKind>((size_t)i, (size_t)npix, S, feat, C, pthi::Counted{samples, E}, K, Side{in...});
}
__global__ __launch_bounds__(kBlock) void k_history_blend_counted(int npix, const float* __restrict__ S, float samples, const float* __restrict__ E,
                                                                  const V4* __restrict__ C, float* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) pthi::blend_pixel((size_t)i, S, pthi::Counted{samples, E}, C, out);
}

__global__ __launch_bounds__(kBlock) void k_history_key(int npix, const V4* __restrict__ feat, const V4* __restrict__ C, const uint8_t* __restrict__ emitter,
                                                        int num_geoms, float min_history, uint32_t* __restrict__ key) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) key[i] = pthi::round_key((size_t)i, (size_t)npix, feat, C, emitter, num_geoms, min_history);
}
// S and E are read and written at list[i]: distinct entries, so no two threads meet.  (An entry outside the tile writes nothing.)
__global__ __launch_bounds__(kBlock) void k_history_merge(int npix, int m, const int32_t* __restrict__ list, const float* __restrict__ Sw, float gf, float* S,
                                                          float* E) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < m && (uint32_t)list[i] < (uint32_t)npix) pthi::merge_entry((size_t)i, list, Sw, gf, S, E);
}

__global__ __launch_bounds__(kBlock) void k_history_probe_keep(int P, int W, int npix, pthi::ProbeGrid pg, const float* __restrict__ S, const V4* __restrict__ feat,
                                                               V4* __restrict__ PK) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s < P) PK[s] = pthi::probe_keep((size_t)pthi::probe_pixel(pg, W, s), (size_t)npix, S, feat);
}
__global__ __launch_bounds__(kBlock) void k_history_probe_list(int P, int W, pthi::ProbeGrid pg, int32_t* __restrict__ list) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s < P) list[s] = pthi::probe_pixel(pg, W, s);
}
// counts: {changed, skipped}, zeroed on the stream before the launch
__global__ __launch_bounds__(kBlock) void k_history_probe_gradient(int P, int W, int npix, pthi::ProbeGrid pg, const V4* __restrict__ PK, const float* __restrict__ Sw,
                                                                   const V4* __restrict__ feat, const uint8_t* __restrict__ moved, int num_geoms,
                                                                   float* __restrict__ L, int* counts) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= P) return;
  const float l = pthi::probe_gradient((size_t)s, (size_t)pthi::probe_pixel(pg, W, s), (size_t)npix, PK[s], Sw, feat, moved, num_geoms);
  L[s] = l;
  if (l > 0.0f) atomicAdd(&counts[0], 1);
  if (l < 0.0f) atomicAdd(&counts[1], 1);
}
__global__ __launch_bounds__(kBlock) void k_history_probe_apply(int W, int R, pthi::ProbeGrid pg, const float* __restrict__ L, const V4* __restrict__ feat,
                                                                const uint8_t* __restrict__ moved, int num_geoms, pthi::ProbeParams P, V4* C) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < W * R) pthi::probe_apply((size_t)i, W, R, pg, L, feat, moved, num_geoms, P, C);
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
  hipLaunchKernelGGL(k_history_capture<pthi::kPlain>, dim3((pixels + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pixels, rgb_sum_dev,
                     reinterpret_cast<const V4*>(planes_dev), static_cast<const V4*>(current_dev), samples, static_cast<V4*>(kept_dev));
  return launched("pt_history_capture");
}
// ... with the variance side: noise_dev the fold's planes, Tf and Df ptnz::fold_scalars' of the folds so far, current_var_dev VC beside
// current_dev (both or neither), kept_var_dev VK.
int pt_history_capture_variance_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const float* planes_dev, const void* current_dev, float samples,
                                       void* kept_dev, const float* noise_dev, float Tf, float Df, const void* current_var_dev, void* kept_var_dev) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum_dev || !planes_dev || !kept_dev || !(samples > 0.0f) || !noise_dev || !(Tf >= 2.0f) || !(Df >= Tf) ||
      !kept_var_dev || !current_dev != !current_var_dev)
    return pt_fail("pt_history_capture_ex: bad argument");
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_history_capture<pthi::kVariance, const V4*, float, float, const V4*, V4*>), dim3((pixels + kBlock - 1) / kBlock), dim3(kBlock), 0, stream,
                     pixels, rgb_sum_dev, reinterpret_cast<const V4*>(planes_dev), static_cast<const V4*>(current_dev), samples, static_cast<V4*>(kept_dev),
                     reinterpret_cast<const V4*>(noise_dev), Tf, Df, static_cast<const V4*>(current_var_dev), static_cast<V4*>(kept_var_dev));
  return launched("pt_history_capture_ex");
}
// ... with the moments side: current_var_dev VC beside current_dev (both or neither), kept_var_dev VK; no fold.
int pt_history_capture_moments_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const float* planes_dev, const void* current_dev, float samples,
                                      void* kept_dev, const void* current_var_dev, void* kept_var_dev) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum_dev || !planes_dev || !kept_dev || !(samples > 0.0f) || !kept_var_dev || !current_dev != !current_var_dev)
    return pt_fail("pt_history_capture_ex: bad argument");
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_history_capture<pthi::kMoments, const V4*, V4*>), dim3((pixels + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pixels,
                     rgb_sum_dev, reinterpret_cast<const V4*>(planes_dev), static_cast<const V4*>(current_dev), samples, static_cast<V4*>(kept_dev),
                     static_cast<const V4*>(current_var_dev), static_cast<V4*>(kept_var_dev));
  return launched("pt_history_capture_ex");
}

int pt_history_reproject_launch(hipStream_t stream, const pthi::View& v, const void* kept_dev, const float* planes_dev, const uint8_t* reject_dev,
                                int num_geoms, const pthi::Params& P, void* current_dev) {
  if (bad_frame(v.W, v.R)) return pt_fail("pt_history_reproject: a tile of %d x %d pixels is not supported", v.W, v.R);
  if (!kept_dev || !planes_dev || !current_dev || (!P.keep_view_dependent && (num_geoms < 0 || (num_geoms > 0 && !reject_dev))))
    return pt_fail("pt_history_reproject: bad argument");
  const int npix = v.W * v.R;
  hipLaunchKernelGGL(k_history_reproject<pthi::kPlain>, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, npix, v, static_cast<const V4*>(kept_dev),
                     reinterpret_cast<const V4*>(planes_dev), reject_dev, num_geoms, P, static_cast<V4*>(current_dev));
  return launched("pt_history_reproject");
}
// ... with the variance or the moments side: kept_var_dev VK, current_var_dev VC.
template <int kKind>
static int reproject_with_launch(hipStream_t stream, const pthi::View& v, const void* kept_dev, const float* planes_dev, const uint8_t* reject_dev,
                                 int num_geoms, const pthi::Params& P, void* current_dev, const void* kept_var_dev, void* current_var_dev) {
  if (bad_frame(v.W, v.R)) return pt_fail("pt_history_reproject_ex: a tile of %d x %d pixels is not supported", v.W, v.R);
  if (!kept_dev || !planes_dev || !current_dev || !kept_var_dev || !current_var_dev ||
      (!P.keep_view_dependent && (num_geoms < 0 || (num_geoms > 0 && !reject_dev))))
    return pt_fail("pt_history_reproject_ex: bad argument");
  const int npix = v.W * v.R;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_history_reproject<kKind, const V4*, V4*>), dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, npix, v,
                     static_cast<const V4*>(kept_dev), reinterpret_cast<const V4*>(planes_dev), reject_dev, num_geoms, P, static_cast<V4*>(current_dev),
                     static_cast<const V4*>(kept_var_dev), static_cast<V4*>(current_var_dev));
  return launched("pt_history_reproject_ex");
}

int pt_history_reproject_variance_launch(hipStream_t stream, const pthi::View& v, const void* kept_dev, const float* planes_dev, const uint8_t* reject_dev,
                                         int num_geoms, const pthi::Params& P, void* current_dev, const void* kept_var_dev, void* current_var_dev) {
  return reproject_with_launch<pthi::kVariance>(stream, v, kept_dev, planes_dev, reject_dev, num_geoms, P, current_dev, kept_var_dev, current_var_dev);
}
int pt_history_reproject_moments_launch(hipStream_t stream, const pthi::View& v, const void* kept_dev, const float* planes_dev, const uint8_t* reject_dev,
                                        int num_geoms, const pthi::Params& P, void* current_dev, const void* kept_var_dev, void* current_var_dev) {
  return reproject_with_launch<pthi::kMoments>(stream, v, kept_dev, planes_dev, reject_dev, num_geoms, P, current_dev, kept_var_dev, current_var_dev);
}

int pt_history_reproject_motion_launch(hipStream_t stream, uint32_t kind, const pthi::View& v, const void* kept_dev, const float* planes_dev,
                                       const uint8_t* reject_dev, int num_geoms, const pthi::Params& P, void* current_dev, const void* kept_var_dev,
                                       void* current_var_dev, const float* table_dev, const uint8_t* kind_dev) {
  const char* who = "pt_history_reproject_ex";
  if (bad_frame(v.W, v.R)) return pt_fail("%s: a tile of %d x %d pixels is not supported", who, v.W, v.R);
  const bool with = kind != 0;
  if (!kept_dev || !planes_dev || !current_dev || num_geoms < 1 || !table_dev || !kind_dev || (!P.keep_view_dependent && !reject_dev) ||
      (kind != 0 && kind != PT_HISTORY_VARIANCE && kind != PT_HISTORY_MOMENTS) || with != (kept_var_dev != nullptr) || with != (current_var_dev != nullptr))
    return pt_fail("%s: bad argument (motion)", who);
  const int npix = v.W * v.R;
  const dim3 grid((npix + kBlock - 1) / kBlock), block(kBlock);
  const V4 *K = static_cast<const V4*>(kept_dev), *feat = reinterpret_cast<const V4*>(planes_dev), *VK = static_cast<const V4*>(kept_var_dev);
  V4 *C = static_cast<V4*>(current_dev), *VC = static_cast<V4*>(current_var_dev);
  if (kind == PT_HISTORY_VARIANCE)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_history_reproject_motion<pthi::kVariance, const V4*, V4*>), grid, block, 0, stream, npix, v, K, feat, reject_dev, num_geoms, P,
                       table_dev, kind_dev, C, VK, VC);
  else if (kind == PT_HISTORY_MOMENTS)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_history_reproject_motion<pthi::kMoments, const V4*, V4*>), grid, block, 0, stream, npix, v, K, feat, reject_dev, num_geoms, P,
                       table_dev, kind_dev, C, VK, VC);
  else
    hipLaunchKernelGGL(k_history_reproject_motion<pthi::kPlain>, grid, block, 0, stream, npix, v, K, feat, reject_dev, num_geoms, P, table_dev, kind_dev, C);
  return launched(who);
}

template <int kKind, bool kMotion>
static void reproject_materials_launch(hipStream_t stream, int npix, const pthi::View& v, const V4* K, const V4* feat, const uint8_t* reject_dev, int num_geoms,
                                       const pthi::Params& P, const float* table_dev, const uint8_t* kind_dev, const float* recolor_dev, const uint8_t* rkind_dev, V4* C,
                                       const V4* VK, V4* VC) {
  const dim3 grid((npix + kBlock - 1) / kBlock), block(kBlock);
  if constexpr (kKind == pthi::kPlain)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_history_reproject_materials<kKind, kMotion>), grid, block, 0, stream, npix, v, K, feat, reject_dev, num_geoms, P, table_dev, kind_dev,
                       recolor_dev, rkind_dev, C);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_history_reproject_materials<kKind, kMotion, const V4*, V4*>), grid, block, 0, stream, npix, v, K, feat, reject_dev, num_geoms, P,
                       table_dev, kind_dev, recolor_dev, rkind_dev, C, VK, VC);
}
// The lookup with PT_HISTORY_MATERIALS: kind as pt_history_reproject_motion_launch takes it; recolor_dev pthi::kRecolorRow floats (16-byte
// aligned) and rkind_dev one byte per geom (num_geoms >= 1); table_dev / kind_dev both null (no geom moved, or no PT_HISTORY_MOTION) or both given.
int pt_history_reproject_materials_launch(hipStream_t stream, uint32_t kind, const pthi::View& v, const void* kept_dev, const float* planes_dev,
                                          const uint8_t* reject_dev, int num_geoms, const pthi::Params& P, void* current_dev, const void* kept_var_dev,
                                          void* current_var_dev, const float* table_dev, const uint8_t* kind_dev, const float* recolor_dev, const uint8_t* rkind_dev) {
  const char* who = "pt_history_reproject_ex";
  if (bad_frame(v.W, v.R)) return pt_fail("%s: a tile of %d x %d pixels is not supported", who, v.W, v.R);
  const bool with = kind != 0, motion = table_dev != nullptr;
  if (!kept_dev || !planes_dev || !current_dev || num_geoms < 1 || !recolor_dev || !rkind_dev || ((uintptr_t)recolor_dev & 15) || motion != (kind_dev != nullptr) ||
      (!P.keep_view_dependent && !reject_dev) || (kind != 0 && kind != PT_HISTORY_VARIANCE && kind != PT_HISTORY_MOMENTS) || with != (kept_var_dev != nullptr) ||
      with != (current_var_dev != nullptr))
    return pt_fail("%s: bad argument (materials)", who);
  const int npix = v.W * v.R;
  const V4 *K = static_cast<const V4*>(kept_dev), *feat = reinterpret_cast<const V4*>(planes_dev), *VK = static_cast<const V4*>(kept_var_dev);
  V4 *C = static_cast<V4*>(current_dev), *VC = static_cast<V4*>(current_var_dev);
  auto go = [&](auto k, auto m) {
    reproject_materials_launch<decltype(k)::value, decltype(m)::value>(stream, npix, v, K, feat, reject_dev, num_geoms, P, table_dev, kind_dev, recolor_dev, rkind_dev, C, VK, VC);
  };
  auto by_motion = [&](auto k) { motion ? go(k, std::true_type{}) : go(k, std::false_type{}); };
  if (kind == PT_HISTORY_VARIANCE) by_motion(std::integral_constant<int, pthi::kVariance>{});
  else if (kind == PT_HISTORY_MOMENTS) by_motion(std::integral_constant<int, pthi::kMoments>{});
  else by_motion(std::integral_constant<int, pthi::kPlain>{});
  return launched(who);
}

// The moments lookup with PT_HISTORY_FEEDBACK: kept_fb_dev FK, current_fb_dev FC; table_dev / kind_dev both null (no geom moved, or
// no PT_HISTORY_MOTION) or both given (num_geoms >= 1).
int pt_history_reproject_feedback_launch(hipStream_t stream, const pthi::View& v, const void* kept_dev, const float* planes_dev, const uint8_t* reject_dev,
                                         int num_geoms, const pthi::Params& P, void* current_dev, const void* kept_var_dev, void* current_var_dev,
                                         const void* kept_fb_dev, void* current_fb_dev, const float* table_dev, const uint8_t* kind_dev) {
  const char* who = "pt_history_reproject_ex";
  if (bad_frame(v.W, v.R)) return pt_fail("%s: a tile of %d x %d pixels is not supported", who, v.W, v.R);
  const bool motion = table_dev != nullptr;
  if (!kept_dev || !planes_dev || !current_dev || !kept_var_dev || !current_var_dev || !kept_fb_dev || !current_fb_dev || motion != (kind_dev != nullptr) ||
      (motion && num_geoms < 1) || (!P.keep_view_dependent && (num_geoms < 0 || (num_geoms > 0 && !reject_dev))))
    return pt_fail("%s: bad argument (feedback)", who);
  const int npix = v.W * v.R;
  hipLaunchKernelGGL(motion ? k_history_reproject_feedback<true> : k_history_reproject_feedback<false>, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, stream,
                     npix, v, static_cast<const V4*>(kept_dev), reinterpret_cast<const V4*>(planes_dev), reject_dev, num_geoms, P, table_dev, kind_dev,
                     static_cast<V4*>(current_dev), static_cast<const V4*>(kept_var_dev), static_cast<V4*>(current_var_dev), static_cast<const V4*>(kept_fb_dev),
                     static_cast<V4*>(current_fb_dev));
  return launched(who);
}

int pt_history_blend_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, float samples, const void* current_dev, float* rgb_avg_dev) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum_dev || !rgb_avg_dev || !(samples > 0.0f)) return pt_fail("pt_history_resolve: bad argument");
  hipLaunchKernelGGL(k_history_blend, dim3((pixels + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pixels, rgb_sum_dev, samples,
                     static_cast<const V4*>(current_dev), rgb_avg_dev);
  return launched("pt_history_resolve");
}

// The counted forms: extra_dev the plane E, `pixels` floats.
int pt_history_capture_counted_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const float* planes_dev, const void* current_dev, float samples,
                                      const float* extra_dev, void* kept_dev) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum_dev || !planes_dev || !kept_dev || !(samples > 0.0f) || !extra_dev) return pt_fail("pt_history_capture: bad argument");
  hipLaunchKernelGGL(k_history_capture_counted<pthi::kPlain>, dim3((pixels + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pixels, rgb_sum_dev,
                     reinterpret_cast<const V4*>(planes_dev), static_cast<const V4*>(current_dev), samples, extra_dev, static_cast<V4*>(kept_dev));
  return launched("pt_history_capture");
}
int pt_history_capture_moments_counted_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const float* planes_dev, const void* current_dev,
                                              float samples, const float* extra_dev, void* kept_dev, const void* current_var_dev, void* kept_var_dev) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum_dev || !planes_dev || !kept_dev || !(samples > 0.0f) || !extra_dev || !kept_var_dev ||
      !current_dev != !current_var_dev)
    return pt_fail("pt_history_capture_ex: bad argument");
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_history_capture_counted<pthi::kMoments, const V4*, V4*>), dim3((pixels + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pixels,
                     rgb_sum_dev, reinterpret_cast<const V4*>(planes_dev), static_cast<const V4*>(current_dev), samples, extra_dev, static_cast<V4*>(kept_dev),
                     static_cast<const V4*>(current_var_dev), static_cast<V4*>(kept_var_dev));
  return launched("pt_history_capture_ex");
}
int pt_history_blend_counted_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, float samples, const float* extra_dev, const void* current_dev,
                                    float* rgb_avg_dev) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum_dev || !rgb_avg_dev || !(samples > 0.0f) || !extra_dev) return pt_fail("pt_history_resolve: bad argument");
  hipLaunchKernelGGL(k_history_blend_counted, dim3((pixels + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pixels, rgb_sum_dev, samples, extra_dev,
                     static_cast<const V4*>(current_dev), rgb_avg_dev);
  return launched("pt_history_resolve");
}

// The history round's key into key_dev (pixels words: pt_adaptive_select_keys) and its merge.  emitter_dev: one byte per geom, read for
// ids 1 .. num_geoms only.
int pt_history_key_launch(hipStream_t stream, int pixels, const float* planes_dev, const void* current_dev, const uint8_t* emitter_dev, int num_geoms,
                          float min_history, uint32_t* key_dev) {
  if (pixels <= 0 || pixels > (1 << 30) || !planes_dev || !key_dev || num_geoms < 0 || (num_geoms > 0 && !emitter_dev) || !(min_history > 0.0f))
    return pt_fail("pt_history_round: bad argument");
  hipLaunchKernelGGL(k_history_key, dim3((pixels + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pixels, reinterpret_cast<const V4*>(planes_dev),
                     static_cast<const V4*>(current_dev), emitter_dev, num_geoms, min_history, key_dev);
  return launched("pt_history_round");
}
int pt_history_merge_launch(hipStream_t stream, int pixels, float* rgb_sum_dev, float* extra_dev, const int32_t* list_dev, int m, const float* group_sum_dev,
                            int group_iters) {
  if (pixels <= 0 || pixels > (1 << 30) || m < 1 || m > pixels || group_iters < 1 || !rgb_sum_dev || !extra_dev || !list_dev || !group_sum_dev)
    return pt_fail("pt_history_round: bad argument");
  hipLaunchKernelGGL(k_history_merge, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pixels, m, list_dev, group_sum_dev, (float)group_iters, rgb_sum_dev,
                     extra_dev);
  return launched("pt_history_round");
}

// The history probes.  pg = pthi::probe_grid(w, rows, phase) with P = pthi::probe_count(pg) >= 1 probes; every index a kernel forms
// lies inside the tile (probe_pixel < w * rows) or the P entries of probe_dev / list_dev / lam_dev / group_sum_dev.
static bool bad_probes(int w, int rows, int phase) { return bad_frame(w, rows) || phase < 0 || phase > 8 || pthi::probe_count(pthi::probe_grid(w, rows, phase)) < 1; }
int pt_history_probe_keep_launch(hipStream_t stream, int w, int rows, int phase, const float* rgb_sum_dev, const float* planes_dev, void* probe_dev) {
  if (bad_probes(w, rows, phase) || !rgb_sum_dev || !planes_dev || !probe_dev) return pt_fail("pt_history_probe_keep: bad argument");
  const pthi::ProbeGrid pg = pthi::probe_grid(w, rows, phase);
  const int P = pthi::probe_count(pg);
  hipLaunchKernelGGL(k_history_probe_keep, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, P, w, w * rows, pg, rgb_sum_dev,
                     reinterpret_cast<const V4*>(planes_dev), static_cast<V4*>(probe_dev));
  return launched("pt_history_probe_keep");
}
int pt_history_probe_list_launch(hipStream_t stream, int w, int rows, int phase, int32_t* list_dev) {
  if (bad_probes(w, rows, phase) || !list_dev) return pt_fail("pt_history_probe_check: bad argument");
  const pthi::ProbeGrid pg = pthi::probe_grid(w, rows, phase);
  const int P = pthi::probe_count(pg);
  hipLaunchKernelGGL(k_history_probe_list, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, P, w, pg, list_dev);
  return launched("pt_history_probe_check");
}
// counts_dev: two int32 {changed, skipped}, zeroed here on the stream
int pt_history_probe_gradient_launch(hipStream_t stream, int w, int rows, int phase, const void* probe_dev, const float* group_sum_dev, const float* planes_dev,
                                     const uint8_t* moved_dev, int num_geoms, float* lam_dev, int* counts_dev) {
  if (bad_probes(w, rows, phase) || !probe_dev || !group_sum_dev || !planes_dev || !lam_dev || !counts_dev || num_geoms < 0 || (num_geoms > 0 && !moved_dev))
    return pt_fail("pt_history_probe_check: bad argument");
  const pthi::ProbeGrid pg = pthi::probe_grid(w, rows, phase);
  const int P = pthi::probe_count(pg);
  if (hipMemsetAsync(counts_dev, 0, 2 * sizeof(int), stream) != hipSuccess) return pt_fail("pt_history_probe_check: clearing the counts failed");
  hipLaunchKernelGGL(k_history_probe_gradient, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, P, w, w * rows, pg, static_cast<const V4*>(probe_dev),
                     group_sum_dev, reinterpret_cast<const V4*>(planes_dev), moved_dev, num_geoms, lam_dev, counts_dev);
  return launched("pt_history_probe_check");
}
int pt_history_probe_apply_launch(hipStream_t stream, int w, int rows, int phase, const float* lam_dev, const float* planes_dev, const uint8_t* moved_dev,
                                  int num_geoms, const pthi::ProbeParams& P, void* current_dev) {
  if (bad_probes(w, rows, phase) || !lam_dev || !planes_dev || !current_dev || num_geoms < 0 || (num_geoms > 0 && !moved_dev) || P.radius < 0 || P.radius > 4)
    return pt_fail("pt_history_probe_check: bad argument");
  const int npix = w * rows;
  hipLaunchKernelGGL(k_history_probe_apply, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, w, rows, pthi::probe_grid(w, rows, phase), lam_dev,
                     reinterpret_cast<const V4*>(planes_dev), moved_dev, num_geoms, P, static_cast<V4*>(current_dev));
  return launched("pt_history_probe_check");
}
int pt_history_probe_options(const char* who, const PtHistoryProbeOptions* opt, pthi::ProbeParams* P) {
  if (const char* msg = pthi::resolve_probe(opt, P)) return pt_fail("%s: %s", who, msg);
  return 0;
}
// What the host forms refuse first: the frame and the phase.
static int probe_frame_check(const char* who, int w, int rows, int phase) {
  if (w <= 0 || rows <= 0 || (int64_t)w * rows > (1ll << 30)) return pt_fail("%s: a tile of %d x %d pixels is not supported", who, w, rows);
  if (phase < 0 || phase > 8) return pt_fail("%s: phase %d is not in 0 .. 8", who, phase);
  return 0;
}

int pt_history_round_options(const char* who, const PtHistoryRoundOptions* opt, pthi::RoundParams* P) {
  if (const char* msg = pthi::resolve_round(opt, P)) return pt_fail("%s: %s", who, msg);
  return 0;
}
// What the host and stage forms of the selection refuse: the frame, the arrays, the options; *cap the list's capacity.
int pt_history_select_check(const char* who, int w, int rows, const float* feature_planes, const uint8_t* emitter_geom, int num_geoms,
                            const PtHistoryRoundOptions* opt, const int32_t* list, const int* fresh, const int* m, pthi::RoundParams* P, int* cap) {
  if (w <= 0 || rows <= 0 || (int64_t)w * rows > (1ll << 30)) return pt_fail("%s: a tile of %d x %d pixels is not supported", who, w, rows);
  if (!feature_planes || !list || !fresh || !m) return pt_fail("%s: null argument", who);
  if (num_geoms < 0 || (num_geoms > 0 && !emitter_geom)) return pt_fail("%s: null emitter_geom for %d geoms", who, num_geoms);
  if (pt_history_round_options(who, opt, P)) return -1;
  *cap = ptad::list_length((double)P->max_fraction, (int64_t)w * rows);
  return 0;
}
// ... and of the merge: the arrays, the list's entries (inside the tile, distinct), the group.
int pt_history_merge_check(const char* who, int pixels, const float* rgb_sum, const float* extra, const int32_t* list, int m, const float* group_sum,
                           int group_iters) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum || !extra || !list || !group_sum) return pt_fail("%s: bad argument", who);
  if (m < 1 || m > pixels || group_iters < 1) return pt_fail("%s: a list of %d out of %d pixels, a group of %d iterations", who, m, pixels, group_iters);
  std::vector<uint8_t> seen((size_t)pixels, 0);
  for (int i = 0; i < m; ++i) {
    if (list[i] < 0 || list[i] >= pixels || seen[(size_t)list[i]]) return pt_fail("%s: list[%d] = %d is outside the tile or repeated", who, i, list[i]);
    seen[(size_t)list[i]] = 1;
  }
  return 0;
}
// extra: every E_p finite and >= 0 (a count of samples)
int pt_history_check_extra(const char* who, int pixels, const float* extra) {
  if (!extra) return pt_fail("%s: null extra", who);
  for (int i = 0; i < pixels; ++i)
    if (!(extra[i] - extra[i] == 0.0f) || extra[i] < 0.0f) return pt_fail("%s: extra[%d] = %g is not finite and >= 0", who, i, (double)extra[i]);
  return 0;
}

int pt_history_check_samples(const char* who, float samples) {
  if (!(samples - samples == 0.0f) || !(samples > 0.0f)) return pt_fail("%s: samples must be finite and positive", who);
  return 0;
}
// The variance describes the folded image: the blend's weights must count the samples the folds counted.
int pt_history_check_fold_samples(const char* who, float samples, int64_t iters) {
  if (samples != (float)iters) return pt_fail("%s: samples %g, but the folds hold %lld iterations: the variance is that of the folded image", who, (double)samples, (long long)iters);
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

extern "C" int pt_history_capture_variance_host(int pixels, const float* noise_planes, int groups, int64_t iters, float samples, const float* current_plane,
                                                const float* current_var, float* kept_var) {
  const char* who = "pt_history_capture_variance_host";
  if (pixels <= 0 || pixels > (1 << 30) || !noise_planes || !kept_var) return pt_fail("%s: bad argument", who);
  if (pt_history_check_samples(who, samples)) return -1;
  if (groups < 2) return pt_fail("%s: %d group(s) folded; a variance needs at least 2 (pt_noise_fold after each group of iterations)", who, groups);
  if (iters < groups) return pt_fail("%s: %d groups cannot hold %lld iterations (every group holds at least one)", who, groups, (long long)iters);
  if (pt_history_check_fold_samples(who, samples, iters)) return -1;
  if (!current_plane != !current_var) return pt_fail("%s: the current plane and its variance come together or not at all", who);
  const ptnz::Fold f = ptnz::fold_scalars(1, groups, iters);
  pthi::capture_variance_host((size_t)pixels, noise_planes, f.Tf, f.Df, samples, current_plane, current_var, kept_var);
  return 0;
}

extern "C" int pt_history_reproject_variance_host(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                                  const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var,
                                                  float* current_plane, float* current_var) {
  pthi::Params P{};
  const char* who = "pt_history_reproject_variance_host";
  if (pt_history_reproject_check(who, w, rows, row0, kept_cam, kept_planes, feature_planes, reject_geom, num_geoms, opt, current_plane, &P)) return -1;
  if (!kept_var || !current_var) return pt_fail("%s: null argument", who);
  pthi::reproject_variance_host(pthi::make_view(*kept_cam, rows, row0), kept_planes, feature_planes, reject_geom, num_geoms, P, kept_var, current_plane, current_var);
  return 0;
}

extern "C" int pt_history_capture_moments_host(int pixels, const float* rgb_sum, float samples, const float* current_plane, const float* current_var,
                                               float* kept_var) {
  const char* who = "pt_history_capture_moments_host";
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum || !kept_var) return pt_fail("%s: bad argument", who);
  if (pt_history_check_samples(who, samples)) return -1;
  if (!current_plane != !current_var) return pt_fail("%s: the current plane and its moments come together or not at all", who);
  pthi::capture_moments_host((size_t)pixels, rgb_sum, samples, current_plane, current_var, kept_var);
  return 0;
}

extern "C" int pt_history_reproject_moments_host(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                                 const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var,
                                                 float* current_plane, float* current_var) {
  pthi::Params P{};
  const char* who = "pt_history_reproject_moments_host";
  if (pt_history_reproject_check(who, w, rows, row0, kept_cam, kept_planes, feature_planes, reject_geom, num_geoms, opt, current_plane, &P)) return -1;
  if (!kept_var || !current_var) return pt_fail("%s: null argument", who);
  pthi::reproject_moments_host(pthi::make_view(*kept_cam, rows, row0), kept_planes, feature_planes, reject_geom, num_geoms, P, kept_var, current_plane, current_var);
  return 0;
}

// ---- the objects' motion (PT_HISTORY_MOTION) -------------------------------------------------------------------------------
extern "C" int pt_history_motion_host(const PtGeom* kept, const PtGeom* cur, int n, float* table, uint8_t* kind) {
  if (!kept || !cur || n <= 0 || !table || !kind) return pt_fail("pt_history_motion_host: bad argument");
  pthi::motion_table(kept, cur, n, table, kind);
  return 0;
}
int pt_history_motion_check(const char* who, uint32_t flags, int num_geoms, const float* table, const uint8_t* kind, const float* kept_var,
                            const float* current_var) {
  constexpr uint32_t defined = PT_HISTORY_VARIANCE | PT_HISTORY_MOMENTS | PT_HISTORY_MOTION;
  if (flags & ~defined) return pt_fail("%s: undefined flag bit(s) 0x%x (defined: PT_HISTORY_VARIANCE, PT_HISTORY_MOMENTS, PT_HISTORY_MOTION)", who, flags & ~defined);
  if ((flags & PT_HISTORY_VARIANCE) && (flags & PT_HISTORY_MOMENTS)) return pt_fail("%s: the flags PT_HISTORY_VARIANCE and PT_HISTORY_MOMENTS exclude each other", who);
  if (num_geoms < 1 || !table || !kind) return pt_fail("%s: a motion table and kinds for at least one geom are needed", who);
  for (int g = 0; g < num_geoms; ++g)
    if (kind[g] > pthi::kCarriesNothing) return pt_fail("%s: kind[%d] = %d is not 0, 1 or 2", who, g, (int)kind[g]);
  if ((flags & (PT_HISTORY_VARIANCE | PT_HISTORY_MOMENTS)) && (!kept_var || !current_var)) return pt_fail("%s: null argument", who);
  return 0;
}
extern "C" int pt_history_reproject_motion_host(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                                const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var,
                                                const float* table, const uint8_t* kind, uint32_t flags, float* current_plane, float* current_var) {
  pthi::Params P{};
  const char* who = "pt_history_reproject_motion_host";
  if (pt_history_reproject_check(who, w, rows, row0, kept_cam, kept_planes, feature_planes, reject_geom, num_geoms, opt, current_plane, &P)) return -1;
  if (pt_history_motion_check(who, flags, num_geoms, table, kind, kept_var, current_var)) return -1;
  const pthi::View v = pthi::make_view(*kept_cam, rows, row0);
  const pthi::Motion mo{table, kind};
  if (flags & PT_HISTORY_VARIANCE) pthi::reproject_motion_host<pthi::kVariance>(v, kept_planes, feature_planes, reject_geom, num_geoms, P, kept_var, mo, current_plane, current_var);
  else if (flags & PT_HISTORY_MOMENTS) pthi::reproject_motion_host<pthi::kMoments>(v, kept_planes, feature_planes, reject_geom, num_geoms, P, kept_var, mo, current_plane, current_var);
  else pthi::reproject_motion_host<pthi::kPlain>(v, kept_planes, feature_planes, reject_geom, num_geoms, P, nullptr, mo, current_plane, nullptr);
  return 0;
}

// ---- the materials' edits (PT_HISTORY_MATERIALS) -----------------------------------------------------------------------------
extern "C" int pt_history_recolor_host(const PtMaterial* kept, const PtMaterial* cur, int num_materials, const PtGeom* geoms, int num_geoms, float* table,
                                       uint8_t* kind) {
  if (!kept || !cur || num_materials <= 0 || !geoms || num_geoms <= 0 || !table || !kind) return pt_fail("pt_history_recolor_host: bad argument");
  pthi::recolor_table(kept, cur, num_materials, geoms, num_geoms, table, kind);
  return 0;
}
int pt_history_materials_check(const char* who, uint32_t flags, int num_geoms, const float* table, const uint8_t* kind, const float* recolor, const uint8_t* rkind,
                               const float* kept_var, const float* current_var) {
  constexpr uint32_t defined = PT_HISTORY_VARIANCE | PT_HISTORY_MOMENTS | PT_HISTORY_MOTION | PT_HISTORY_MATERIALS;
  if (flags & ~defined)
    return pt_fail("%s: undefined flag bit(s) 0x%x (defined: PT_HISTORY_VARIANCE, PT_HISTORY_MOMENTS, PT_HISTORY_MOTION, PT_HISTORY_MATERIALS)", who, flags & ~defined);
  if ((flags & PT_HISTORY_VARIANCE) && (flags & PT_HISTORY_MOMENTS)) return pt_fail("%s: the flags PT_HISTORY_VARIANCE and PT_HISTORY_MOMENTS exclude each other", who);
  if (num_geoms < 1 || !recolor || !rkind) return pt_fail("%s: a recolour table and kinds for at least one geom are needed", who);
  if (((flags & PT_HISTORY_MOTION) && (!table || !kind)) || (!table != !kind)) return pt_fail("%s: the motion table and its kinds come together, and with PT_HISTORY_MOTION", who);
  for (int g = 0; g < num_geoms; ++g)
    if (rkind[g] > pthi::kCarriesNothing || (kind && kind[g] > pthi::kCarriesNothing))
      return pt_fail("%s: kind[%d] = %d (motion) or %d (recolour) is not 0, 1 or 2", who, g, kind ? (int)kind[g] : 0, (int)rkind[g]);
  if ((flags & (PT_HISTORY_VARIANCE | PT_HISTORY_MOMENTS)) && (!kept_var || !current_var)) return pt_fail("%s: null argument", who);
  return 0;
}
extern "C" int pt_history_reproject_materials_host(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                                   const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var,
                                                   const float* table, const uint8_t* kind, const float* recolor, const uint8_t* rkind, uint32_t flags,
                                                   float* current_plane, float* current_var) {
  pthi::Params P{};
  const char* who = "pt_history_reproject_materials_host";
  if (pt_history_reproject_check(who, w, rows, row0, kept_cam, kept_planes, feature_planes, reject_geom, num_geoms, opt, current_plane, &P)) return -1;
  if (pt_history_materials_check(who, flags, num_geoms, table, kind, recolor, rkind, kept_var, current_var)) return -1;
  const pthi::View v = pthi::make_view(*kept_cam, rows, row0);
  const pthi::Motion mo{table, kind};
  const pthi::Motion* mop = table ? &mo : nullptr;
  const pthi::Recolor rc{recolor, rkind};
  if (flags & PT_HISTORY_VARIANCE) pthi::reproject_materials_host<pthi::kVariance>(v, kept_planes, feature_planes, reject_geom, num_geoms, P, kept_var, mop, rc, current_plane, current_var);
  else if (flags & PT_HISTORY_MOMENTS) pthi::reproject_materials_host<pthi::kMoments>(v, kept_planes, feature_planes, reject_geom, num_geoms, P, kept_var, mop, rc, current_plane, current_var);
  else pthi::reproject_materials_host<pthi::kPlain>(v, kept_planes, feature_planes, reject_geom, num_geoms, P, nullptr, mop, rc, current_plane, nullptr);
  return 0;
}

// What the host and stage forms of the lookup with feedback refuse after pt_history_reproject_check: the planes, then a table without
// kinds (or the reverse) and a kind that is none.
int pt_history_reproject_feedback_check(const char* who, int num_geoms, const float* kept_var, const float* kept_fb, const float* table, const uint8_t* kind,
                                        const float* current_var, const float* current_fb) {
  if (!kept_var || !kept_fb || !current_var || !current_fb) return pt_fail("%s: null argument", who);
  if (!table != !kind) return pt_fail("%s: the motion table and the kinds come together or not at all", who);
  if (table && num_geoms < 1) return pt_fail("%s: a motion table and kinds for at least one geom are needed", who);
  for (int g = 0; table && g < num_geoms; ++g)
    if (kind[g] > pthi::kCarriesNothing) return pt_fail("%s: kind[%d] = %d is not 0, 1 or 2", who, g, (int)kind[g]);
  return 0;
}
extern "C" int pt_history_reproject_feedback_host(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                                  const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var,
                                                  const float* kept_fb, const float* table, const uint8_t* kind, float* current_plane, float* current_var,
                                                  float* current_fb) {
  pthi::Params P{};
  const char* who = "pt_history_reproject_feedback_host";
  if (pt_history_reproject_check(who, w, rows, row0, kept_cam, kept_planes, feature_planes, reject_geom, num_geoms, opt, current_plane, &P)) return -1;
  if (pt_history_reproject_feedback_check(who, num_geoms, kept_var, kept_fb, table, kind, current_var, current_fb)) return -1;
  const pthi::Motion mo{table, kind};
  pthi::reproject_feedback_host(pthi::make_view(*kept_cam, rows, row0), kept_planes, feature_planes, reject_geom, num_geoms, P, kept_var, kept_fb,
                                table ? &mo : nullptr, current_plane, current_var, current_fb);
  return 0;
}

extern "C" int pt_history_blend_host(int pixels, const float* rgb_sum, float samples, const float* current_plane, float* rgb_avg) {
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum || !rgb_avg) return pt_fail("pt_history_blend_host: bad argument");
  if (pt_history_check_samples("pt_history_blend_host", samples)) return -1;
  pthi::blend_host((size_t)pixels, rgb_sum, samples, current_plane, rgb_avg);
  return 0;
}

// ---- the history round on the host ---------------------------------------------------------------------------------------
extern "C" int pt_history_select_host(int w, int rows, const float* feature_planes, const float* current_plane, const uint8_t* emitter_geom, int num_geoms,
                                      const PtHistoryRoundOptions* opt, int32_t* list, int* fresh, int* m) {
  pthi::RoundParams P{};
  int cap = 0;
  if (pt_history_select_check("pt_history_select_host", w, rows, feature_planes, emitter_geom, num_geoms, opt, list, fresh, m, &P, &cap)) return -1;
  pthi::select_host((size_t)w * rows, feature_planes, current_plane, emitter_geom, num_geoms, P.min_history, cap, list, fresh, m);
  return 0;
}
extern "C" int pt_history_merge_host(int pixels, float* rgb_sum, float* extra, const int32_t* list, int m, const float* group_sum, int group_iters) {
  if (pt_history_merge_check("pt_history_merge_host", pixels, rgb_sum, extra, list, m, group_sum, group_iters)) return -1;
  pthi::merge_host(rgb_sum, extra, list, m, group_sum, group_iters);
  return 0;
}
extern "C" int pt_history_blend_counted_host(int pixels, const float* rgb_sum, float samples, const float* extra, const float* current_plane, float* rgb_avg) {
  const char* who = "pt_history_blend_counted_host";
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum || !rgb_avg) return pt_fail("%s: bad argument", who);
  if (pt_history_check_samples(who, samples) || pt_history_check_extra(who, pixels, extra)) return -1;
  pthi::blend_counted_host((size_t)pixels, rgb_sum, samples, extra, current_plane, rgb_avg);
  return 0;
}
extern "C" int pt_history_capture_counted_host(int pixels, const float* rgb_sum, const float* feature_planes, const float* current_plane, float samples,
                                               const float* extra, float* kept_planes) {
  const char* who = "pt_history_capture_counted_host";
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum || !feature_planes || !kept_planes) return pt_fail("%s: bad argument", who);
  if (pt_history_check_samples(who, samples) || pt_history_check_extra(who, pixels, extra)) return -1;
  pthi::capture_counted_host((size_t)pixels, rgb_sum, feature_planes, current_plane, samples, extra, kept_planes);
  return 0;
}
extern "C" int pt_history_capture_moments_counted_host(int pixels, const float* rgb_sum, float samples, const float* extra, const float* current_plane,
                                                       const float* current_var, float* kept_var) {
  const char* who = "pt_history_capture_moments_counted_host";
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum || !kept_var) return pt_fail("%s: bad argument", who);
  if (pt_history_check_samples(who, samples) || pt_history_check_extra(who, pixels, extra)) return -1;
  if (!current_plane != !current_var) return pt_fail("%s: the current plane and its moments come together or not at all", who);
  pthi::capture_moments_counted_host((size_t)pixels, rgb_sum, samples, extra, current_plane, current_var, kept_var);
  return 0;
}

// ---- the history probes on the host ---------------------------------------------------------------------------------------
extern "C" int pt_history_probe_list_host(int w, int rows, int phase, int32_t* list, int* count) {
  const char* who = "pt_history_probe_list_host";
  if (probe_frame_check(who, w, rows, phase)) return -1;
  if (!count) return pt_fail("%s: null count", who);
  const pthi::ProbeGrid pg = pthi::probe_grid(w, rows, phase);
  *count = pthi::probe_count(pg);
  for (int s = 0; list && s < *count; ++s) list[s] = pthi::probe_pixel(pg, w, s);
  return 0;
}
extern "C" int pt_history_probe_keep_host(int w, int rows, int phase, const float* rgb_sum, const float* feature_planes, float* kept) {
  const char* who = "pt_history_probe_keep_host";
  if (probe_frame_check(who, w, rows, phase)) return -1;
  const int P = pthi::probe_count(pthi::probe_grid(w, rows, phase));
  if (!rgb_sum || !feature_planes || (P > 0 && !kept)) return pt_fail("%s: null argument", who);
  pthi::probe_keep_host(w, rows, phase, rgb_sum, feature_planes, kept);
  return 0;
}
extern "C" int pt_history_probe_gradient_host(int w, int rows, int phase, const float* kept, const float* group_sum, const float* feature_planes,
                                              const uint8_t* moved_geom, int num_geoms, float* lam, int* changed, int* skipped) {
  const char* who = "pt_history_probe_gradient_host";
  if (probe_frame_check(who, w, rows, phase)) return -1;
  const int P = pthi::probe_count(pthi::probe_grid(w, rows, phase));
  if (!feature_planes || (P > 0 && (!kept || !group_sum || !lam))) return pt_fail("%s: null argument", who);
  if (num_geoms < 0 || (num_geoms > 0 && !moved_geom)) return pt_fail("%s: null moved_geom for %d geoms", who, num_geoms);
  pthi::probe_gradient_host(w, rows, phase, kept, group_sum, feature_planes, moved_geom, num_geoms, lam, changed, skipped);
  return 0;
}
extern "C" int pt_history_probe_apply_host(int w, int rows, int phase, const float* lam, const float* feature_planes, const uint8_t* moved_geom, int num_geoms,
                                           const PtHistoryProbeOptions* opt, float* current_plane) {
  const char* who = "pt_history_probe_apply_host";
  if (probe_frame_check(who, w, rows, phase)) return -1;
  const int P = pthi::probe_count(pthi::probe_grid(w, rows, phase));
  if (!feature_planes || !current_plane || (P > 0 && !lam)) return pt_fail("%s: null argument", who);
  if (num_geoms < 0 || (num_geoms > 0 && !moved_geom)) return pt_fail("%s: null moved_geom for %d geoms", who, num_geoms);
  pthi::ProbeParams pp{};
  if (pt_history_probe_options(who, opt, &pp)) return -1;
  pthi::probe_apply_host(w, rows, phase, lam, feature_planes, moved_geom, num_geoms, pp, current_plane);
  return 0;
}
