// pt_denoise.hip — the kernels of the edge-avoiding à-trous filter (include/pt_amd.h pt_denoise) and their launcher.
//
// A translation unit of its own, compiled ONCE with -ffp-contract=off: the filter is specified as separate IEEE float32 operations
// (pt_denoise.h), so there is nothing an arithmetic mode could change, and the path tracer's kernels (pt_kernels.hip) are not
// rebuilt differently because of it.  The kernels are thin: thread indices in, the PT_HD bodies of pt_denoise.h, which the host
// loop (ptdn::denoise_host, behind the pt_denoise*_host entry points) runs too.  Five templates, eleven kernels, and four for the
// history round and the feedback, listed after them (ptdn::Form: Plain =
// pt_denoise, Guided = pt_denoise_guided, Adaptive = pt_denoise_adaptive, History = pt_history_denoise, Moments = pt_history_denoise_ex
// with PT_HISTORY_MOMENTS):
//
//   k_denoise_prepare<Form>        one thread per pixel: SUM image + feature SUM planes -> normal | hit, position, albedo, colour (4 x 16 B)
//                                  <Guided>: + the two noise planes in, var_raw out in the albedo's spare word
//                                  <Adaptive>: <Guided> with the pixel's own counts (8 B more in; the count plane, or the fold's two
//                                  scalars in the uniform state), Tf_p out in the position's spare word
//                                  <History>: <Guided> over the blend with the reprojected history: + 16 B of C and 16 B of VC in (when
//                                  present); per pixel 12 B of S, 48 B of features, 32 B of noise, 16 + 16 B of history in, 64 B out
//                                  <Moments>: the blend and its variance from the history's moments, no noise planes: per pixel 12 B of
//                                  S, 48 B of features, 16 + 16 B of history in, 64 B out; var_raw = -1 marks a pixel for the next kernel
//                                  <HistoryAdaptive> (pt_history_denoise_adaptive): <History> with the pixel's own counts as <Adaptive>
//                                  reads them (8 B more in) and Tf_p for the blend's samples; NE_p = Tf_p + Th out in the position's spare
//                                  word, so that k_denoise_var_prefilter<true> and everything behind it run unchanged
//   k_denoise_prepare_counted      <Moments> while the history round's extra plane is present (pt_history_round): + 4 B of E in per pixel,
//                                  the pixel's samples are samples + E_p; a twelfth kernel, launched only then
//   k_denoise_var_spatial          the moments form, between prepare and the prefilter; the level kernel's shape (64 x 4 tiles, a wave is
//                                  64 pixels of a row).  A wave with no marked lane leaves on a ballot of the mark (4 B per lane read):
//                                  how many do is the frame's affair (misses are always marked).  A marked lane walks its 7 x 7 neighbourhood, 3 x 16 B per tap
//                                  (n, p, c), rows outer; neighbouring lanes read neighbouring pixels (1 KiB per wave and load when all
//                                  are marked, as on the first view), the 7-fold reuse between rows and columns is L1's and L2's; no
//                                  LDS.  Writes the lane's own a.w only
//   k_denoise_var_prefilter<bool>  the guided forms; one thread per pixel, 64 x 4 tiles: 3 x 3 over var_raw and the hit flags, var_0 into
//                                  colour buffer 0's .w.  <true>, the adaptive form: over var_raw * Tf of the nine neighbours (n.w, a.w,
//                                  p.w), back in the centre's unit
//   k_denoise_level<bool>          the hot path, once per level: a 64 x 4 workgroup, lanes along x (at every step consecutive lanes read
//                                  consecutive pixels: 1 KiB per wave and load), each thread kRows pixels of its column, rows s apart
//                                  (pt_denoise.h level_column_of); no LDS, the reuse left between neighbouring columns is L1's and L2's
//                                  <true>, the guided forms: the same shape and loads (the variance rides in the colour's .w); per centre
//                                  two more registers (its colour factor, the sum of w^2 var), per tap a multiply and a multiply-add
//   k_denoise_finish               one thread per pixel: remodulation, 12 B per pixel
// The feedback form (Feedback = pt_history_denoise_feedback) runs the moments form's kernels between two of its own:
//   k_denoise_prepare_feedback<bool>  <Moments> with 16 B of FC more in per pixel (when present): the colour is the blend with the FILTERED
//                                  history; var_raw from the raw chain, or from FC.w by option.  <true>: counted, 4 B of E more in
//   k_history_feedback_tap         after level L - 1, one thread per pixel, streaming: 16 B of c_L and 16 B of the albedo buffer in, 16 B of
//                                  the pending plane P out (48 B per pixel); no LDS
#include <hip/hip_runtime.h>

#include "pt_denoise.h"
#include "pt_internal.h"
#include "pt_noise.h"

namespace {
using ptdn::Divisors;
using ptdn::Form;
using ptdn::Params;
using ptdn::V4;
constexpr int kBlock = 256;
constexpr int kLevelX = 64, kLevelY = kBlock / kLevelX;  // a wave is 64 pixels of one row slot

// What a form's prepare takes between the planes and keep_albedo: the noise planes and the members of ptdn::Divisors that it reads.
// They arrive as the kernel arguments In..., one per member in this order, so that every form's arguments are the scalars, at the
// offsets, that its kernel took when the three were written out (a struct argument is loaded in other pieces).
template <Form>
struct PrepareIn {
  float Tf;
};
template <>
struct PrepareIn<Form::Guided> {
  const V4* __restrict__ noise;
  float Tf, Df;
};
template <>
struct PrepareIn<Form::Adaptive> {
  const V4* __restrict__ noise;
  const ptad::Cnt* __restrict__ cnt;
  int T, M;
};
template <>
struct PrepareIn<Form::History> {
  const V4* __restrict__ noise;
  const V4* __restrict__ C;
  const V4* __restrict__ VC;
  float Tf, Df, samples;
};
template <>
struct PrepareIn<Form::HistoryAdaptive> {
  const V4* __restrict__ noise;
  const ptad::Cnt* __restrict__ cnt;
  const V4* __restrict__ C;
  const V4* __restrict__ VC;
  int T, M;
};
template <>
struct PrepareIn<Form::Moments> {
  const V4* __restrict__ C;
  const V4* __restrict__ VC;
  float samples;
};
template <Form kForm, typename... In>
__global__ __launch_bounds__(kBlock) void k_denoise_prepare(int npix, const float* __restrict__ S, const V4* __restrict__ planes, In... in, int keep_albedo,
                                                            V4* __restrict__ n, V4* __restrict__ p, V4* __restrict__ a, V4* __restrict__ c) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const PrepareIn<kForm> d{in...};
  const V4* noise = nullptr;
  if constexpr (kForm != Form::Plain && kForm != Form::Moments) noise = d.noise;
  if (i < npix) ptdn::prepare_pixel_of<kForm>((size_t)i, (size_t)npix, S, planes, noise, d, keep_albedo, n, p, a, c);
}

// The moments form's prepare while the history round's extra plane E is present: 4 B of E more per pixel in, ns = samples + E_p for
// `samples`.  A kernel of its own, so that k_denoise_prepare<Moments> keeps its arguments and its code.
struct PrepareInCounted {
  const V4* __restrict__ C;
  const V4* __restrict__ VC;
  float samples;
  const float* __restrict__ E;
};
__global__ __launch_bounds__(kBlock) void k_denoise_prepare_counted(int npix, const float* __restrict__ S, const V4* __restrict__ planes, const V4* __restrict__ C,
                                                                    const V4* __restrict__ VC, float samples, const float* __restrict__ E, int keep_albedo,
                                                                    V4* __restrict__ n, V4* __restrict__ p, V4* __restrict__ a, V4* __restrict__ c) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const PrepareInCounted d{C, VC, samples, E};
  if (i < npix) ptdn::prepare_pixel_of<Form::Moments>((size_t)i, (size_t)npix, S, planes, nullptr, d, keep_albedo, n, p, a, c);
}

// The feedback form's prepare: kernels of their own, so that the moments form's keep their arguments and their code.
struct PrepareInFeedback {
  const V4* __restrict__ C;
  const V4* __restrict__ VC;
  const V4* __restrict__ FC;
  float samples;
  int fb_variance;
};
struct PrepareInFeedbackCounted {
  const V4* __restrict__ C;
  const V4* __restrict__ VC;
  const V4* __restrict__ FC;
  float samples;
  int fb_variance;
  const float* __restrict__ E;
};
template <bool kCounted>
__global__ __launch_bounds__(kBlock) void k_denoise_prepare_feedback(int npix, const float* __restrict__ S, const V4* __restrict__ planes, const V4* __restrict__ C,
                                                                     const V4* __restrict__ VC, const V4* __restrict__ FC, float samples, int fb_variance,
                                                                     const float* __restrict__ E, int keep_albedo, V4* __restrict__ n, V4* __restrict__ p,
                                                                     V4* __restrict__ a, V4* __restrict__ c) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= npix) return;
  if constexpr (kCounted) {
    const PrepareInFeedbackCounted d{C, VC, FC, samples, fb_variance, E};
    ptdn::prepare_pixel_of<Form::Feedback>((size_t)i, (size_t)npix, S, planes, nullptr, d, keep_albedo, n, p, a, c);
  } else {
    const PrepareInFeedback d{C, VC, FC, samples, fb_variance};
    ptdn::prepare_pixel_of<Form::Feedback>((size_t)i, (size_t)npix, S, planes, nullptr, d, keep_albedo, n, p, a, c);
  }
}
// The tap: the pending plane P from c_L and the albedo buffer
__global__ __launch_bounds__(kBlock) void k_history_feedback_tap(int npix, int keep_albedo, const V4* __restrict__ c, const V4* __restrict__ a,
                                                                 pthi::V4* __restrict__ tap) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) ptdn::tap_pixel((size_t)i, keep_albedo, c, a, tap);
}

// `a` is read (the lane's own mark) and written (the lane's own var_raw): no __restrict__ promise is needed or made for it.
__global__ __launch_bounds__(kBlock) void k_denoise_var_spatial(int W, int R, Params P, const V4* __restrict__ n, const V4* __restrict__ p,
                                                                const V4* __restrict__ c, V4* a) {
  const int x = blockIdx.x * kLevelX + (threadIdx.x & (kLevelX - 1));
  const int y = blockIdx.y * kLevelY + threadIdx.x / kLevelX;
  const bool marked = x < W && y < R && ptdn::spatial_marked(a[(size_t)y * W + x].w);
  if (__ballot(marked) == 0) return;  // wave-uniform: no lane of this wave has anything to do
  if (marked) ptdn::var_spatial_pixel(W, R, x, y, P, n, p, c, a);
}

template <bool kAdaptive>
__global__ __launch_bounds__(kBlock) void k_denoise_var_prefilter(int W, int R, const V4* __restrict__ n, const V4* __restrict__ a,
                                                                  const V4* __restrict__ p, V4* __restrict__ c0) {
  const int x = blockIdx.x * kLevelX + (threadIdx.x & (kLevelX - 1));
  const int y = blockIdx.y * kLevelY + threadIdx.x / kLevelX;
  if (x < W && y < R) ptdn::var_prefilter_of<kAdaptive>(W, R, x, y, n, a, p, c0);
}

template <bool kGuided>
__global__ __launch_bounds__(kBlock) void k_denoise_level(int W, int R, int l, Params P, const V4* __restrict__ c, const V4* __restrict__ n,
                                                          const V4* __restrict__ p, V4* __restrict__ out) {
  const int x = blockIdx.x * kLevelX + (threadIdx.x & (kLevelX - 1));
  const int ty = blockIdx.y * kLevelY + threadIdx.x / kLevelX;
  if (x < W && ty < ptdn::level_slots(R, l)) ptdn::level_column_of<kGuided>(W, R, x, ty, l, P, c, n, p, out);
}

__global__ __launch_bounds__(kBlock) void k_denoise_finish(int npix, int keep_albedo, const V4* __restrict__ c, const V4* __restrict__ a,
                                                           float* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) ptdn::finish_pixel((size_t)i, keep_albedo, c, a, out);
}

}  // namespace

// pt_internal.h.  Everything is checked before the first launch; no allocation, no synchronisation.
int pt_denoise_launch(hipStream_t stream, const ptdn::Job& j, void* workspace_dev, const float** rgb_avg_dev) {
  static const char* const kWho[] = {"pt_denoise", "pt_denoise_guided", "pt_denoise_adaptive", "pt_history_denoise", "pt_history_denoise_ex",
                                     "pt_history_denoise_feedback", "pt_history_denoise_adaptive"};
  const char* who = kWho[(int)j.form];
  const int w = j.f.w, rows = j.f.rows;
  const Params& P = j.P;
  const Divisors& d = j.div;
  if (w <= 0 || rows <= 0 || rows >= 32768 || (int64_t)w * rows > (1ll << 30)) return pt_fail("%s: a frame of %d x %d pixels is not supported", who, w, rows);
  const bool ok = j.form == Form::Plain      ? d.Tf > 0.0f
                  : j.form == Form::Guided   ? j.f.noise && d.Tf >= 2.0f && d.Df >= d.Tf
                  : j.form == Form::Adaptive ? j.f.noise && (d.cnt || (d.M >= 2 && d.T >= d.M))
                  : j.form == Form::HistoryAdaptive ? j.f.noise && (d.cnt || (d.M >= 2 && d.T >= d.M)) && !d.C == !d.VC
                  : j.form == Form::Moments  ? d.samples > 0.0f && !d.C == !d.VC
                  : j.form == Form::Feedback ? d.samples > 0.0f && !d.C == !d.VC && !d.C == !d.FC && (d.fb_variance == 0 || d.fb_variance == 1) && j.tap &&
                                                   j.tap_level >= 1 && j.tap_level <= P.levels
                                             : j.f.noise && d.Tf >= 2.0f && d.Df >= d.Tf && d.samples > 0.0f && !d.C == !d.VC;
  if (!j.f.rgb_sum || !j.f.planes || !workspace_dev || !ok || (d.E && j.form != Form::Moments && j.form != Form::Feedback) || P.levels < 1 || P.levels > ptdn::kMaxLevels) return pt_fail("%s: bad argument", who);
  const int npix = w * rows;
  V4* n = static_cast<V4*>(workspace_dev);
  V4 *p = n + npix, *a = p + npix, *col[2] = {a + npix, a + 2 * (size_t)npix};
  const int flat = (npix + kBlock - 1) / kBlock;
  const dim3 tiles((w + kLevelX - 1) / kLevelX, (rows + kLevelY - 1) / kLevelY);
  const bool blend_counts = j.form == Form::HistoryAdaptive;
  const bool guided = j.form != Form::Plain, adaptive = j.form == Form::Adaptive, history = j.form == Form::History, feedback = j.form == Form::Feedback,
             moments = j.form == Form::Moments || feedback;
  const V4 *planes = reinterpret_cast<const V4*>(j.f.planes), *noise = reinterpret_cast<const V4*>(j.f.noise);
  if (adaptive)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_denoise_prepare<Form::Adaptive, const V4* __restrict__, const ptad::Cnt* __restrict__, int, int>), dim3(flat), dim3(kBlock),
                       0, stream, npix, j.f.rgb_sum, planes, noise, d.cnt, d.T, d.M, P.keep_albedo, n, p, a, col[0]);
  else if (blend_counts)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_denoise_prepare<Form::HistoryAdaptive, const V4* __restrict__, const ptad::Cnt* __restrict__, const V4* __restrict__,
                                                         const V4* __restrict__, int, int>),
                       dim3(flat), dim3(kBlock), 0, stream, npix, j.f.rgb_sum, planes, noise, d.cnt, d.C, d.VC, d.T, d.M, P.keep_albedo, n, p, a, col[0]);
  else if (history)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_denoise_prepare<Form::History, const V4* __restrict__, const V4* __restrict__, const V4* __restrict__, float, float, float>),
                       dim3(flat), dim3(kBlock), 0, stream, npix, j.f.rgb_sum, planes, noise, d.C, d.VC, d.Tf, d.Df, d.samples, P.keep_albedo, n, p, a, col[0]);
  else if (feedback && d.E)
    hipLaunchKernelGGL(k_denoise_prepare_feedback<true>, dim3(flat), dim3(kBlock), 0, stream, npix, j.f.rgb_sum, planes, d.C, d.VC, d.FC, d.samples, d.fb_variance, d.E,
                       P.keep_albedo, n, p, a, col[0]);
  else if (feedback)
    hipLaunchKernelGGL(k_denoise_prepare_feedback<false>, dim3(flat), dim3(kBlock), 0, stream, npix, j.f.rgb_sum, planes, d.C, d.VC, d.FC, d.samples, d.fb_variance,
                       static_cast<const float*>(nullptr), P.keep_albedo, n, p, a, col[0]);
  else if (moments && d.E)
    hipLaunchKernelGGL(k_denoise_prepare_counted, dim3(flat), dim3(kBlock), 0, stream, npix, j.f.rgb_sum, planes, d.C, d.VC, d.samples, d.E, P.keep_albedo, n, p, a,
                       col[0]);
  else if (moments)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_denoise_prepare<Form::Moments, const V4* __restrict__, const V4* __restrict__, float>), dim3(flat), dim3(kBlock), 0, stream,
                       npix, j.f.rgb_sum, planes, d.C, d.VC, d.samples, P.keep_albedo, n, p, a, col[0]);
  else if (guided)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_denoise_prepare<Form::Guided, const V4* __restrict__, float, float>), dim3(flat), dim3(kBlock), 0, stream, npix, j.f.rgb_sum,
                       planes, noise, d.Tf, d.Df, P.keep_albedo, n, p, a, col[0]);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_denoise_prepare<Form::Plain, float>), dim3(flat), dim3(kBlock), 0, stream, npix, j.f.rgb_sum, planes, d.Tf, P.keep_albedo, n, p,
                       a, col[0]);
  if (moments) hipLaunchKernelGGL(k_denoise_var_spatial, tiles, dim3(kBlock), 0, stream, w, rows, P, n, p, col[0], a);
  if (guided)
    hipLaunchKernelGGL(adaptive || blend_counts ? k_denoise_var_prefilter<true> : k_denoise_var_prefilter<false>, tiles, dim3(kBlock), 0, stream, w, rows, n, a, p, col[0]);
  for (int l = 0; l < P.levels; ++l) {
    const dim3 grid(tiles.x, (ptdn::level_slots(rows, l) + kLevelY - 1) / kLevelY);
    hipLaunchKernelGGL(guided ? k_denoise_level<true> : k_denoise_level<false>, grid, dim3(kBlock), 0, stream, w, rows, l, P, col[ptdn::color_buffer(l)], n, p,
                       col[ptdn::color_buffer(l + 1)]);
    if (feedback && l + 1 == j.tap_level)
      hipLaunchKernelGGL(k_history_feedback_tap, dim3(flat), dim3(kBlock), 0, stream, npix, P.keep_albedo, col[ptdn::color_buffer(l + 1)], a,
                         static_cast<pthi::V4*>(j.tap));
  }
  float* out = reinterpret_cast<float*>(col[ptdn::color_buffer(P.levels + 1)]);
  hipLaunchKernelGGL(k_denoise_finish, dim3(flat), dim3(kBlock), 0, stream, npix, P.keep_albedo, col[ptdn::color_buffer(P.levels)], a, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pt_fail("%s: launch failed: %s", who, hipGetErrorString(e));
  if (rgb_avg_dev) *rgb_avg_dev = out;
  return 0;
}

// pt_internal.h.  Plain: samples.  Guided: the fold counters M = groups, T = iters -> ptnz::fold_scalars' Tf, Df.  Adaptive: (T, M) for
// every pixel of the uniform state; whoever has a count plane sets div.cnt afterwards.  History: the guided form's two and samples;
// whoever has the planes C and VC sets div.C and div.VC (a launch) or f.current and f.current_var (the host loop) afterwards.
// Moments: samples alone, and the planes likewise.
int pt_denoise_resolve(const char* who, ptdn::Form form, float samples, int groups, int64_t iters, const PtDenoiseOptions* opt, ptdn::Job* j) {
  if (form == Form::Plain && !(samples > 0.0f)) return pt_fail("%s: samples must be positive", who);
  if (form == Form::Guided || form == Form::History) {
    if (groups < 2) return pt_fail("%s: %d group(s) folded; a variance needs at least 2 (pt_noise_fold after each group of iterations)", who, groups);
    if (iters < groups) return pt_fail("%s: %d groups cannot hold %lld iterations (every group holds at least one)", who, groups, (long long)iters);
  }
  *j = ptdn::Job{};
  j->form = form;
  const bool blended = form == Form::History || form == Form::Moments || form == Form::Feedback || form == Form::HistoryAdaptive;
  if (const char* msg = ptdn::resolve(opt, &j->P, form == Form::Plain ? 4.0f : blended ? ptdn::kHistorySigmaColor : ptdn::kGuidedSigmaColor)) return pt_fail("%s: %s", who, msg);
  if (form == Form::Plain) j->div.Tf = samples;
  if (blended) j->div.samples = samples;
  if (form == Form::Guided || form == Form::History) {
    const ptnz::Fold f = ptnz::fold_scalars(1, groups, iters);
    j->div.Tf = f.Tf, j->div.Df = f.Df;
  }
  if (form == Form::Adaptive || form == Form::HistoryAdaptive) j->div.T = (int32_t)iters, j->div.M = groups;
  return 0;
}

int pt_denoise_adaptive_check(const char* who, int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                              const PtDenoiseOptions* opt, ptdn::Job* j) {
  if (w <= 0 || rows <= 0 || (int64_t)w * rows > (1ll << 30)) return pt_fail("%s: a frame of %d x %d pixels is not supported", who, w, rows);
  if (!rgb_sum || !planes || !noise_planes || !counts) return pt_fail("%s: null argument", who);
  const size_t npix = (size_t)w * rows;
  for (size_t i = 0; i < npix; ++i)
    if (counts[2 * i + 1] < 2 || counts[2 * i] < counts[2 * i + 1])
      return pt_fail("%s: pixel %zu has T = %d iterations in M = %d groups; a variance needs M >= 2 and T >= M", who, i, counts[2 * i], counts[2 * i + 1]);
  return pt_denoise_resolve(who, Form::Adaptive, 0.0f, 0, 0, opt, j);
}

// What the host and stage forms of the history filter refuse, in the order of pt_history_denoise: the arrays' shape, samples, the options,
// the folds' counters, samples != (float)iters, C without VC, a null output.
int pt_history_denoise_check(const char* who, int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups, int64_t iters,
                             float samples, const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, const float* rgb_avg, ptdn::Job* j) {
  if (w <= 0 || rows <= 0 || (int64_t)w * rows > (1ll << 30)) return pt_fail("%s: a frame of %d x %d pixels is not supported", who, w, rows);
  if (!rgb_sum || !planes || !noise_planes) return pt_fail("%s: null argument", who);
  if (pt_history_check_samples(who, samples)) return -1;
  ptdn::Params P{};  // (the options before the folds' counters: pt_denoise_resolve alone would look at the counters first)
  if (const char* msg = ptdn::resolve(opt, &P, ptdn::kHistorySigmaColor)) return pt_fail("%s: %s", who, msg);
  if (pt_denoise_resolve(who, Form::History, samples, groups, iters, opt, j)) return -1;
  if (pt_history_check_fold_samples(who, samples, iters)) return -1;
  if (!current_plane != !current_var)
    return pt_fail("%s: the current plane %s its variance: both or neither (a lookup made with PT_HISTORY_VARIANCE gives both)", who,
                   current_plane ? "comes without" : "is absent, but not");
  if (!rgb_avg) return pt_fail("%s: null buffer", who);
  return 0;
}

// ... and of the history form with per-pixel counts: the arrays' shape and the counts (pt_denoise_adaptive_check's words), the options, C
// without VC, no output.
int pt_history_denoise_adaptive_check(const char* who, int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                                      const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, bool has_output, ptdn::Job* j) {
  if (pt_denoise_adaptive_check(who, w, rows, rgb_sum, planes, noise_planes, counts, opt, j)) return -1;
  if (pt_denoise_resolve(who, Form::HistoryAdaptive, 0.0f, 0, 0, opt, j)) return -1;
  if (!current_plane != !current_var)
    return pt_fail("%s: the current plane %s its variance: both or neither (a lookup made with PT_HISTORY_VARIANCE gives both)", who,
                   current_plane ? "comes without" : "is absent, but not");
  if (!has_output) return pt_fail("%s: null buffer", who);
  return 0;
}

// ... and of the moments form, in pt_history_denoise_ex's order: the arrays' shape, samples, the options, C without VC, no output.
int pt_history_denoise_moments_check(const char* who, int w, int rows, const float* rgb_sum, const float* planes, float samples, const float* current_plane,
                                     const float* current_var, const PtDenoiseOptions* opt, bool has_output, ptdn::Job* j) {
  if (w <= 0 || rows <= 0 || (int64_t)w * rows > (1ll << 30)) return pt_fail("%s: a frame of %d x %d pixels is not supported", who, w, rows);
  if (!rgb_sum || !planes) return pt_fail("%s: null argument", who);
  if (pt_history_check_samples(who, samples)) return -1;
  if (pt_denoise_resolve(who, Form::Moments, samples, 0, 0, opt, j)) return -1;
  if (!current_plane != !current_var)
    return pt_fail("%s: the current plane %s its moments: both or neither (a lookup made with PT_HISTORY_MOMENTS gives both)", who,
                   current_plane ? "comes without" : "is absent, but not");
  if (!has_output) return pt_fail("%s: null buffer", who);
  return 0;
}

// ... and of the feedback form (pt_internal.h): the moments form's in their order, then fb out of range and C without FC.
int pt_history_feedback_options(const char* who, const PtHistoryFeedbackOptions* fb, int levels, int* level, int* variance) {
  PtHistoryFeedbackOptions o{};
  if (fb) o = *fb;
  if (o.level == 0) o.level = PT_HISTORY_FEEDBACK_LEVEL;
  if (o.level < 1 || o.level > levels) return pt_fail("%s: feedback level %d is not in 1 .. %d (the filter's levels)", who, o.level, levels);
  if (o.variance < -1 || o.variance > 1) return pt_fail("%s: feedback variance %d is not 1, or -1 for rule 0", who, o.variance);
  if (o.variance == 0) o.variance = PT_HISTORY_FEEDBACK_VARIANCE;
  if (o.variance == -1) o.variance = 0;
  *level = o.level, *variance = o.variance;
  return 0;
}
int pt_history_denoise_feedback_check(const char* who, int w, int rows, const float* rgb_sum, const float* planes, float samples, const float* current_plane,
                                      const float* current_var, const float* current_fb, const PtDenoiseOptions* opt, const PtHistoryFeedbackOptions* fb,
                                      bool has_output, ptdn::Job* j) {
  if (pt_history_denoise_moments_check(who, w, rows, rgb_sum, planes, samples, current_plane, current_var, opt, has_output, j)) return -1;
  j->form = Form::Feedback;
  if (pt_history_feedback_options(who, fb, j->P.levels, &j->tap_level, &j->div.fb_variance)) return -1;
  if (!current_plane != !current_fb)
    return pt_fail("%s: the current plane %s its filtered colour: both or neither (a lookup made with PT_HISTORY_FEEDBACK gives both)", who,
                   current_plane ? "comes without" : "is absent, but not");
  return 0;
}

namespace {
// The host entry points: what they refuse (the adaptive form: pt_denoise_adaptive_check), then the one host loop.  want_avg: rgb_avg
// is the output (the variance variants have none and ask for no level).
int host_filter(const char* who, Form form, int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                float samples, int groups, int64_t iters, const PtDenoiseOptions* opt, bool want_avg, float* rgb_avg, float* var_raw, float* var_0) {
  ptdn::Job j{};
  if (form == Form::Adaptive) {
    if (want_avg && !rgb_avg) return pt_fail("%s: null argument", who);
    if (pt_denoise_adaptive_check(who, w, rows, rgb_sum, planes, noise_planes, counts, opt, &j)) return -1;
  } else {
    if (w <= 0 || rows <= 0 || (int64_t)w * rows > (1ll << 30) || !rgb_sum || !planes || (form != Form::Plain && !noise_planes) || (want_avg && !rgb_avg))
      return pt_fail("%s: bad argument", who);
    if (pt_denoise_resolve(who, form, samples, groups, iters, opt, &j)) return -1;
  }
  j.f = {w, rows, rgb_sum, planes, noise_planes};
  ptdn::denoise_host(j, counts, rgb_avg, var_raw, var_0);
  return 0;
}
}  // namespace

extern "C" {
int pt_denoise_host(int w, int rows, const float* rgb_sum, const float* planes, float samples, const PtDenoiseOptions* opt, float* rgb_avg) {
  return host_filter("pt_denoise_host", Form::Plain, w, rows, rgb_sum, planes, nullptr, nullptr, samples, 0, 0, opt, true, rgb_avg, nullptr, nullptr);
}
int pt_denoise_guided_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups, int64_t iters,
                           const PtDenoiseOptions* opt, float* rgb_avg) {
  return host_filter("pt_denoise_guided_host", Form::Guided, w, rows, rgb_sum, planes, noise_planes, nullptr, 0.0f, groups, iters, opt, true, rgb_avg, nullptr, nullptr);
}
int pt_denoise_guided_variance_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups, int64_t iters,
                                    const PtDenoiseOptions* opt, float* var_raw, float* var_0) {
  return host_filter("pt_denoise_guided_variance_host", Form::Guided, w, rows, rgb_sum, planes, noise_planes, nullptr, 0.0f, groups, iters, opt, false, nullptr,
                     var_raw, var_0);
}
int pt_history_denoise_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups, int64_t iters, float samples,
                            const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, float* rgb_avg) {
  ptdn::Job j{};
  if (pt_history_denoise_check("pt_history_denoise_host", w, rows, rgb_sum, planes, noise_planes, groups, iters, samples, current_plane, current_var, opt, rgb_avg, &j))
    return -1;
  j.f = {w, rows, rgb_sum, planes, noise_planes, current_plane, current_var};
  ptdn::denoise_host(j, nullptr, rgb_avg);
  return 0;
}
int pt_history_denoise_moments_host(int w, int rows, const float* rgb_sum, const float* planes, float samples, const float* current_plane,
                                    const float* current_var, const PtDenoiseOptions* opt, float* rgb_avg, float* var_raw, uint8_t* mark) {
  ptdn::Job j{};
  if (pt_history_denoise_moments_check("pt_history_denoise_moments_host", w, rows, rgb_sum, planes, samples, current_plane, current_var, opt,
                                       rgb_avg || var_raw || mark, &j))
    return -1;
  j.f = {w, rows, rgb_sum, planes, nullptr, current_plane, current_var};
  ptdn::denoise_host(j, nullptr, rgb_avg, var_raw, nullptr, mark);
  return 0;
}
int pt_history_denoise_moments_counted_host(int w, int rows, const float* rgb_sum, const float* planes, float samples, const float* extra,
                                            const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, float* rgb_avg,
                                            float* var_raw, uint8_t* mark) {
  const char* who = "pt_history_denoise_moments_counted_host";
  ptdn::Job j{};
  if (pt_history_denoise_moments_check(who, w, rows, rgb_sum, planes, samples, current_plane, current_var, opt, rgb_avg || var_raw || mark, &j)) return -1;
  if (pt_history_check_extra(who, w * rows, extra)) return -1;
  j.f = {w, rows, rgb_sum, planes, nullptr, current_plane, current_var, extra};
  ptdn::denoise_host(j, nullptr, rgb_avg, var_raw, nullptr, mark);
  return 0;
}
int pt_history_denoise_feedback_host(int w, int rows, const float* rgb_sum, const float* planes, float samples, const float* extra, const float* current_plane,
                                     const float* current_var, const float* current_fb, const PtDenoiseOptions* opt, const PtHistoryFeedbackOptions* fb,
                                     float* rgb_avg, float* tap, float* var_raw, uint8_t* mark) {
  const char* who = "pt_history_denoise_feedback_host";
  ptdn::Job j{};
  if (pt_history_denoise_feedback_check(who, w, rows, rgb_sum, planes, samples, current_plane, current_var, current_fb, opt, fb,
                                        rgb_avg || tap || var_raw || mark, &j))
    return -1;
  if (extra && pt_history_check_extra(who, w * rows, extra)) return -1;
  j.f = {w, rows, rgb_sum, planes, nullptr, current_plane, current_var, extra, current_fb};
  j.tap = tap;
  ptdn::denoise_host(j, nullptr, rgb_avg, var_raw, nullptr, mark);
  return 0;
}
int pt_history_denoise_adaptive_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                                     const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, float* rgb_avg) {
  ptdn::Job j{};
  if (pt_history_denoise_adaptive_check("pt_history_denoise_adaptive_host", w, rows, rgb_sum, planes, noise_planes, counts, current_plane, current_var, opt,
                                        rgb_avg != nullptr, &j))
    return -1;
  j.f = {w, rows, rgb_sum, planes, noise_planes, current_plane, current_var};
  ptdn::denoise_host(j, counts, rgb_avg);
  return 0;
}
int pt_history_denoise_adaptive_variance_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                                              const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, float* var_raw, float* var_0) {
  ptdn::Job j{};
  if (pt_history_denoise_adaptive_check("pt_history_denoise_adaptive_variance_host", w, rows, rgb_sum, planes, noise_planes, counts, current_plane, current_var, opt,
                                        var_raw || var_0, &j))
    return -1;
  j.f = {w, rows, rgb_sum, planes, noise_planes, current_plane, current_var};
  ptdn::denoise_host(j, counts, nullptr, var_raw, var_0);
  return 0;
}
int pt_denoise_adaptive_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                             const PtDenoiseOptions* opt, float* rgb_avg) {
  return host_filter("pt_denoise_adaptive_host", Form::Adaptive, w, rows, rgb_sum, planes, noise_planes, counts, 0.0f, 0, 0, opt, true, rgb_avg, nullptr, nullptr);
}
int pt_denoise_adaptive_variance_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                                      const PtDenoiseOptions* opt, float* var_raw, float* var_0) {
  return host_filter("pt_denoise_adaptive_variance_host", Form::Adaptive, w, rows, rgb_sum, planes, noise_planes, counts, 0.0f, 0, 0, opt, false, nullptr, var_raw,
                     var_0);
}
}  // extern "C"
