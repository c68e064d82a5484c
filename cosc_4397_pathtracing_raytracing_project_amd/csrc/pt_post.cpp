// pt_post.cpp — what reads or extends a rendered image, on a context (pt_context.h): the first-hit feature buffers, the two
// edge-avoiding filters, the noise estimate and render-until, adaptive sampling with its worker context, and resolve.  The kernels
// are pt_features.inc (through KernelApi), pt_denoise.hip, pt_noise.hip, pt_adaptive.hip, pt_history.hip and (a striped tile's list) pt_group_select.hip; this file holds their host side: what
// an entry point refuses, the buffers that exist from the first use on, and the launches.
#include <cmath>
#include <cstring>

#include "pt_adaptive.h"
#include "pt_context.h"
#include "pt_denoise.h"
#include "pt_history.h"
#include "pt_noise.h"
#include "pt_sched.h"

using namespace ptc;

// pt_internal.h (pt_group_denoise_guided: the group refuses what its contexts would refuse, before anything is exchanged)
int64_t pt_ctx_unfolded_iterations(const PtContext* c) { return c ? c->rendered - c->noise_iters : 0; }

extern "C" {

// ---- first-hit feature buffers (csrc/pt_features.inc) --------------------------------------------
int pt_ctx_render_features(PtContext* c, int iter_first, int iter_count) {
  if (need(c, "pt_render_features")) return -1;
  Ctx& g = *c;
  if (iter_first < 1 || iter_count < 0 || (int64_t)iter_first + iter_count - 1 > INT32_MAX)
    return pt_fail("pt_render_features: iterations %d, +%d: the first is >= 1, the count >= 0", iter_first, iter_count);
  if (admit(g, "pt_render_features", kNotFailed | kOnDevice)) return -1;
  const ptk::SceneTables sc = tables(g);
  static_assert(sizeof(float4) == 16, "a feature plane holds 16 bytes per pixel");
  if (ensure(g, g.d_feat, (size_t)PT_FEATURE_PLANES * g.N * sizeof(float4), Zero::on_stream)) return -1;  // the first feature pass of the context
  if (iter_count == 0) return 0;
  // one wave per group of 64 pixels, no more workgroups than are resident (the table placement can differ between calls: debug grids)
  const int groups = (g.N + 63) / 64;
  g.grid_features = std::min((groups + ptk::kWavesPerBlock - 1) / ptk::kWavesPerBlock,
                             g.num_cus * std::min(g.cap_bpc, g.k->resident_blocks_per_cu(ptk::kFeatures, sc)));
  g.k->features(g.stream, g.grid_features, sc, g.dcam, tile_batch(g, iter_first, iter_count), g.d_feat);
  HIP_OK(hipGetLastError());
  g.feat_fresh = true;
  g.fb_pending = false;  // the feedback's pending plane was filtered along other features
  return 0;
}

int pt_ctx_readback_features(PtContext* c, float* planes_host) {
  if (need(c, "pt_readback_features")) return -1;
  return copy_out(c, "pt_readback_features", planes_host, 4 * PT_FEATURE_PLANES, [&](const float** d) {
    return (*d = pt_ctx_device_features(c)) ? 0 : pt_fail("pt_readback_features: no feature pass has been rendered (pt_render_features)");
  });
}

const float* pt_ctx_device_features(PtContext* c) { return c ? reinterpret_cast<const float*>(c->d_feat) : nullptr; }

// ---- edge-avoiding filter over the image and the feature buffers (csrc/pt_denoise.hip) ------------------------
// One body for the three forms.  The guided forms run on the same tile and in the same workspace, plus the planes of the noise estimate
// — which must describe the image as it is, so iterations rendered since the last fold are refused rather than filtered with a stale
// variance.  The adaptive form is the guided filter with the sample counts of every pixel, so the one filter that runs in the adaptive
// state (the count plane) as well as in the uniform state (the fold's counters for every pixel, as pt_readback_adaptive reports them).
static int denoise_device(PtContext* c, const char* who, ptdn::Form form, float samples, const PtDenoiseOptions* opt, const float** rgb_dev) {
  const bool plain = form == ptdn::Form::Plain, adaptive = form == ptdn::Form::Adaptive;
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (admit(g, who, kNotFailed | (adaptive ? 0u : kUniform) | kNoExtras | kWholeRows)) return -1;
  const int W = g.cam.resolution[0];
  if (!g.d_feat) return pt_fail("%s: no feature pass has been rendered (pt_render_features)", who);
  if (!plain) {
    if (!g.d_noise || g.noise_groups < 1) return pt_fail("%s: nothing has been folded (pt_noise_fold)", who);
    if (admit(g, who, kFoldedAll)) return -1;
  }
  if (adaptive) {
    if (g.noise_groups < 2) return pt_fail("%s: %d group(s) folded; a variance needs at least 2 (pt_noise_fold after each group of iterations)", who, g.noise_groups);
    if (g.noise_iters > INT32_MAX) return pt_fail("%s: %lld iterations folded: the per-pixel counts are int32", who, (long long)g.noise_iters);
  }
  ptdn::Job j{};
  if (pt_denoise_resolve(who, form, samples, g.noise_groups, g.noise_iters, opt, &j)) return -1;
  HIP_OK(hipSetDevice(g.device));
  if (ensure(g, g.d_denoise, pt_denoise_workspace_bytes((size_t)g.N))) return -1;  // the first denoise call of the context, of any kind
  j.f = {W, g.N / W, g.d_image, reinterpret_cast<const float*>(g.d_feat), plain ? nullptr : static_cast<const float*>(g.d_noise)};
  j.div.cnt = adaptive && g.adaptive ? static_cast<const ptad::Cnt*>(g.d_acnt) : nullptr;
  return pt_denoise_launch(g.stream, j, g.d_denoise, rgb_dev);
}
int pt_ctx_denoise_device(PtContext* c, float samples, const PtDenoiseOptions* opt, const float** rgb_dev) {
  return denoise_device(c, "pt_denoise", ptdn::Form::Plain, samples, opt, rgb_dev);
}
int pt_ctx_denoise(PtContext* c, float samples, const PtDenoiseOptions* opt, float* rgb_avg_host) {
  return copy_out(c, "pt_denoise", rgb_avg_host, 3, [&](const float** d) { return pt_ctx_denoise_device(c, samples, opt, d); });
}
int pt_ctx_denoise_guided_device(PtContext* c, const PtDenoiseOptions* opt, const float** rgb_dev) {
  return denoise_device(c, "pt_denoise_guided", ptdn::Form::Guided, 0.0f, opt, rgb_dev);
}
int pt_ctx_denoise_guided(PtContext* c, const PtDenoiseOptions* opt, float* rgb_avg_host) {
  return copy_out(c, "pt_denoise_guided", rgb_avg_host, 3, [&](const float** d) { return pt_ctx_denoise_guided_device(c, opt, d); });
}
int pt_ctx_denoise_adaptive_device(PtContext* c, const PtDenoiseOptions* opt, const float** rgb_dev) {
  return denoise_device(c, "pt_denoise_adaptive", ptdn::Form::Adaptive, 0.0f, opt, rgb_dev);
}
int pt_ctx_denoise_adaptive(PtContext* c, const PtDenoiseOptions* opt, float* rgb_avg_host) {
  return copy_out(c, "pt_denoise_adaptive", rgb_avg_host, 3, [&](const float** d) { return pt_ctx_denoise_adaptive_device(c, opt, d); });
}

// ---- noise estimate from batch sums, render until a target PSNR (csrc/pt_noise.hip) ----------------------------
int pt_ctx_noise_fold(PtContext* c) {
  if (need(c, "pt_noise_fold")) return -1;
  Ctx& g = *c;
  if (admit(g, "pt_noise_fold", kNotFailed | kUniform | kNoExtras)) return -1;
  const int64_t n = g.rendered - g.noise_iters;
  if (n <= 0) return 0;  // nothing rendered since the last fold
  HIP_OK(hipSetDevice(g.device));
  if (ensure(g, g.d_noise, pt_noise_state_bytes((size_t)g.N), Zero::on_stream)) return -1;  // the first fold of the context: zeroed like the image it starts from
  if (pt_noise_launch(g.stream, g.N, g.d_image, g.d_noise, ptnz::fold_scalars(n, g.noise_groups + 1, g.noise_iters + n))) return -1;
  g.noise_groups += 1;
  g.noise_iters += n;
  return 0;
}

int pt_ctx_get_noise(PtContext* c, double* sse, int* groups, int* iterations) {
  if (need(c, "pt_get_noise")) return -1;
  if (pt_ctx_sync(c)) return -1;
  Ctx& g = *c;
  if (sse) {
    *sse = -1.0;
    if (g.d_noise && g.noise_groups >= 2) {
      const char* result = static_cast<const char*>(g.d_noise) + pt_noise_state_bytes((size_t)g.N) - sizeof(double);
      HIP_OK(hipMemcpy(sse, result, sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  // (the adaptive state: the last merge's SSE_est lies where a fold's does; every round counts as a group)
  if (groups) *groups = g.noise_groups + g.adaptive_rounds;
  if (iterations) *iterations = (int)std::min<int64_t>(g.adaptive ? g.adaptive_last : g.noise_iters, INT32_MAX);
  return 0;
}

int pt_ctx_readback_noise(PtContext* c, float* planes_host) {
  if (need(c, "pt_readback_noise")) return -1;
  return copy_out(c, "pt_readback_noise", planes_host, 4 * PT_NOISE_PLANES, [&](const float** d) {
    return (*d = pt_ctx_device_noise(c)) ? 0 : pt_fail("pt_readback_noise: nothing has been folded (pt_noise_fold)");
  });
}

const float* pt_ctx_device_noise(PtContext* c) { return c ? static_cast<const float*>(c->d_noise) : nullptr; }

int pt_ctx_render_until(PtContext* c, int iter_first, int max_iters, int group_iters, float target_db, int* iters_done, float* psnr_db) {
  if (need(c, "pt_render_until")) return -1;
  Ctx& g = *c;
  if (iter_first < 1 || max_iters < 1 || (int64_t)iter_first + max_iters - 1 > INT32_MAX || group_iters < 0 || !std::isfinite(target_db))
    return pt_fail("pt_render_until: iterations %d, +%d in groups of %d until %g dB: the first is >= 1, the count >= 1, the group >= 0 (0 = a batch), the target finite",
                iter_first, max_iters, group_iters, (double)target_db);
  if (admit(g, "pt_render_until", kNotFailed | kUniform | kNoExtras)) return -1;
  const int group = group_iters ? group_iters : g.K;
  int done = 0;
  float psnr = -1.0f;
  while (done < max_iters) {
    const int n = std::min(group, max_iters - done);
    if (pt_ctx_render(c, iter_first + done, n)) return -1;
    done += n;
    double sse = -1.0;
    if (pt_ctx_noise_fold(c) || pt_ctx_get_noise(c, &sse, nullptr, nullptr)) return -1;
    if (sse < 0.0) continue;  // one group says nothing about the spread
    psnr = pt_psnr_from_sse(sse, g.N);
    if (psnr > target_db) break;
  }
  if (iters_done) *iters_done = done;
  if (psnr_db) *psnr_db = psnr;
  return 0;
}

}  // extern "C"

// Threshold rounds over the blend (further down): the keys of passes A and B into the selection's workspace, and what those rounds refuse
// after the adaptive rounds' own refusals.
extern "C" {
static int history_blend_keys(PtContext& g);
static int history_threshold_refusal(const PtContext& g, const char* who);
}

// ---- adaptive sampling: further groups over the noisiest pixels only (csrc/pt_adaptive.hip) -------------------------------
namespace ptc {
// A round over m <= capacity pixels on a worker planned for `capacity`: only what follows from N is planned again — the chunks per
// queue, the paths per queue and batch, the record slots per region (pt_sched.h queue_plan).  K, Q, slot_shift, the launch widths and
// every buffer stay those of the capacity: queue_plan is monotone in N for fixed Q and K (tests/test_sched_capacity.py), so the
// smaller plan's regions lie inside the larger one's, and the path buffers keep their plane distance (PathBuf::stride, an allocation's
// property).  Nothing is freed, allocated or cleared; the retirement fill levels and the counter rows are zero between batches anyway.
void set_worker_live(Ctx& w, int m) {
  const ptk::QueuePlan plan = ptk::queue_plan(m, w.qs.Q, w.K);
  w.N = m;
  w.qs.nq = plan.nq;
  w.qs.inv_nq = 1.0f / (float)plan.nq;
  w.qs.cap = plan.cap;
  w.stride = (int64_t)w.qs.Q * plan.cap;
  w.ret.seg_cap = plan.seg_cap;
}

// The worker context for a list of up to m pixels: batches, queues, buffers and launch widths planned for N = m like any context's; the
// scene tables, the grid or BVH choice and the LDS-table decision are the parent's (neither uploaded nor measured again, not owned).
// A worker of that capacity is kept, with its live size back at the capacity; one of another capacity is replaced.
int ensure_worker(Ctx& g, int m) {
  if (g.worker && g.worker->capacity == m) return set_worker_live(*g.worker, m), 0;
  if (g.worker) g.device_bytes -= g.worker->device_bytes, destroy(g.worker), g.worker = nullptr;
  if (ensure(g, g.d_list, (size_t)g.N * sizeof(int32_t), Zero::blocking)) return -1;  // the list: every entry a tile pixel from the start
  // A striped tile: the kernels read a list entry as an offset from pixel_begin in the FRAME (pt_kernels.hip global_pixel), the merge as
  // a TILE index; the worker gets a second list, derived from the first on the device (round_list).  A contiguous tile: one buffer.
  if (g.stripe && ensure(g, g.d_list_frame, (size_t)g.N * sizeof(int32_t), Zero::blocking)) return -1;
  Ctx* w = new Ctx();
  w->borrowed = true;
  static_cast<PtShared&>(*w) = g;
  PtOptions o{};
  o.pixel_begin = g.pixel_begin, o.pixel_count = m;
  o.iters_per_batch = g.opt_iters_per_batch, o.num_queues = g.opt_num_queues;  // 0: automatic for m pixels
  if (plan_batches(*w, o)) return destroy(w), -1;
  plan_launch(*w);
  if (alloc_batch_buffers(*w)) return destroy(w), -1;
  w->list = g.stripe ? g.d_list_frame : g.d_list;
  w->capacity = m;
  g.worker = w;
  g.device_bytes += w->device_bytes;
  return 0;
}

// Iterations iter_first .. iter_first + iter_count - 1 of the listed pixels into the worker's cleared group sum.
int render_list(Ctx& g, int iter_first, int iter_count) {
  Ctx& w = *g.worker;
  w.primary_valid = false;  // a round's list is new behind the same pointer: depth 0 is traced once per round (pt_sched.h BatchForm::primary_once)
  HIP_OK(hipMemsetAsync(w.d_image, 0, 3 * (size_t)w.N * sizeof(float), g.stream));
  const int end = iter_first + iter_count;
  for (int it = iter_first; it < end; it += w.K)
    if (run_batch(w, it, std::min(w.K, end - it))) {
      g.failed = true;
      return -1;
    }
  return 0;
}

// Everything a round refuses, before anything is allocated or launched.  pt_render_adaptive asks with folds == false: without the
// state of the folds, which its uniform groups establish, and with its own words about the first iteration (its group may be 0).
// A round over a caller's list has no fraction (nullptr) and needs no rows (rows == false); a group's round has the fraction, and its
// contexts' tiles are rows dealt in turn.
static int adaptive_refusal(const Ctx& g, const char* who, int iter_first, int group_iters, const float* fraction_or_null, bool folds = true,
                            bool rows = true) {
  const float fraction = fraction_or_null ? *fraction_or_null : 1.0f;
  if (admit(g, who, kNotFailed | kNoExtras)) return -1;  // (the history round's extras: the counts of a round are the folds')
  if (folds && (iter_first < 1 || group_iters < 1 || (int64_t)iter_first + group_iters - 1 > INT32_MAX))
    return pt_fail("%s: iterations %d, +%d: the first is >= 1, the group holds at least one", who, iter_first, group_iters);
  if (!folds && iter_first < 1) return pt_fail("%s: the first iteration %d is not >= 1", who, iter_first);
  if (!(fraction > 0.0f && fraction <= 1.0f)) return pt_fail("%s: fraction %g is not in (0, 1]", who, (double)fraction);
  if (g.conv) return pt_fail("%s: the renderer was created with PtOptions.convergence = %d; the convergence metric follows whole iterations", who, g.conv);
  if (rows && admit(g, who, kWholeRows)) return -1;
  if (g.adaptive || !folds) return 0;
  if (g.noise_groups < 2) return pt_fail("%s: %d group(s) folded; the selection needs the noise estimate of at least 2 (pt_noise_fold)", who, g.noise_groups);
  if (admit(g, who, kFoldedAll)) return -1;
  if (g.noise_iters > INT32_MAX / 2) return pt_fail("%s: %lld iterations folded: the per-pixel counts are int32", who, (long long)g.noise_iters);
  return 0;
}

// The first round since pt_init / pt_clear, of any kind: every pixel has the fold's T and M.  (The selection's workspace belongs to
// the rounds that select: a round over a caller's list has none.)
static int enter_adaptive(Ctx& g) {
  if (g.adaptive) return 0;
  if (ensure(g, g.d_acnt, (size_t)g.N * sizeof(ptad::Cnt))) return -1;
  if (pt_adaptive_init_counts_launch(g.stream, g.N, g.d_acnt, (int)g.noise_iters, g.noise_groups)) return -1;
  g.adaptive = true;
  g.adaptive_rounds = 0;
  g.adaptive_last = g.noise_iters;
  return 0;
}

// The second half of a round: the worker's live tile renders the group, the merge joins it.
static int render_and_merge(Ctx& g, int iter_first, int group_iters, int m) {
  if (render_list(g, iter_first, group_iters)) return -1;
  if (pt_adaptive_merge_launch(g.stream, g.N, g.d_image, g.d_noise, g.d_acnt, g.d_list, m, g.worker->d_image, group_iters)) return -1;
  g.adaptive_rounds += 1;
  g.adaptive_last = std::max<int64_t>(g.adaptive_last, (int64_t)iter_first + group_iters - 1);
  g.samples += (int64_t)group_iters * m;  // (live_rays and the kernel timings stay the parent's own launches')
  g.hist_noise = g.hist_ne = false;  // the blend's W and NE described the image that was
  return 0;
}

// A threshold round after its refusals: key and select, the two counts read back (8 bytes and ONE synchronise, which a fixed-fraction
// round does not have: the list's length decides the launches that follow), then the group over the first m entries unless
// above <= min_pixels.  *selected: the pixels rendered, 0 when nothing was.  blend (pt_history_round_threshold): the keys are those of the
// blend's variance (history_blend_keys) in place of k_adaptive_key's; everything behind the keys is the same.
static int threshold_round(Ctx& g, const char* who, bool blend, int iter_first, int group_iters, float threshold, float max_fraction, int min_pixels, int* above,
                           int* selected) {
  HIP_OK(hipSetDevice(g.device));
  const int W = g.cam.resolution[0];
  if (enter_adaptive(g) || ensure(g, g.d_select, pt_adaptive_select_bytes((size_t)g.N))) return -1;
  const int cap = ptad::list_length((double)max_fraction, g.N);
  if (ensure_worker(g, cap)) return -1;
  if (blend ? history_blend_keys(g) || pt_adaptive_select_threshold_keys_launch(g.stream, W, g.N / W, threshold, cap, g.d_select, g.d_list)
            : pt_adaptive_select_threshold_launch(g.stream, W, g.N / W, static_cast<const float*>(g.d_noise), g.d_acnt, threshold, cap, g.d_select, g.d_list))
    return -1;
  uint32_t result[2] = {0u, 0u};  // above, m
  HIP_OK(hipMemcpyAsync(result, pt_adaptive_select_result(g.d_select, (size_t)g.N), sizeof(result), hipMemcpyDeviceToHost, g.stream));
  HIP_OK(hipStreamSynchronize(g.stream));
  const int m = (int)result[1];
  if (m < 0 || m > cap || (int)result[0] < m) return pt_fail("%s: the selection left %u above, a list of %u (cap %d)", who, result[0], result[1], cap);
  const bool render = m > 0 && (int)result[0] > min_pixels;
  if (above) *above = (int)result[0];
  if (selected) *selected = render ? m : 0;
  if (!render) return 0;  // nothing rendered or merged, no round counted, SSE_est where it was
  set_worker_live(*g.worker, m);
  return render_and_merge(g, iter_first, group_iters, m);
}

// A round over a caller's list after its refusals: a pt_adaptive_round without the selection.  `list` lies on the host (host == true:
// uploaded on the context's stream, from pageable memory, so the call returns once the entries have left the caller's array) or on
// the context's device; either way it is copied into the context's own list behind whatever still reads that, and nothing synchronises.
static int round_list(Ctx& g, int iter_first, int group_iters, const int32_t* list, bool host, int m, int capacity) {
  HIP_OK(hipSetDevice(g.device));
  if (enter_adaptive(g) || ensure_worker(g, capacity)) return -1;
  if (m == 0) {  // nothing rendered or merged, SSE_est where it was; the round and its iterations count, so that a group's contexts stay in step
    g.adaptive_rounds += 1;
    g.adaptive_last = std::max<int64_t>(g.adaptive_last, (int64_t)iter_first + group_iters - 1);
    return 0;
  }
  set_worker_live(*g.worker, m);
  HIP_OK(hipMemcpyAsync(g.d_list, list, (size_t)m * sizeof(int32_t), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, g.stream));
  if (g.stripe && pt_group_offsets_launch(g.stream, g.d_list, m, g.stripe, g.stripe_stride - g.stripe, g.d_list_frame)) return -1;
  return render_and_merge(g, iter_first, group_iters, m);
}

static int round_list_entry(PtContext* c, const char* who, int iter_first, int group_iters, const int32_t* list, bool host, int m, int capacity) {
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (adaptive_refusal(g, who, iter_first, group_iters, nullptr, true, false)) return -1;
  if (capacity < 1 || capacity > g.N || m < 0 || m > capacity)
    return pt_fail("%s: a list of %d on a worker for %d out of %d pixels: the capacity is 1 .. the tile, the list 0 .. the capacity", who, m, capacity, g.N);
  if (m > 0 && !list) return pt_fail("%s: null list", who);
  for (int i = 0; host && i < m; ++i)
    if (list[i] < 0 || list[i] >= g.N || (i > 0 && list[i] <= list[i - 1]))
      return pt_fail("%s: list[%d] = %d is outside the tile or not above its predecessor", who, i, list[i]);
  return round_list(g, iter_first, group_iters, list, host, m, capacity);
}
}  // namespace ptc

// pt_context.h: what a group asks of its contexts
PtCtxState pt_ctx_state(const PtContext* c) {
  PtCtxState s{};
  if (c) s.adaptive = c->adaptive, s.groups = c->noise_groups, s.iters = c->noise_iters, s.unfolded = c->rendered - c->noise_iters;
  return s;
}
int pt_ctx_adaptive_refusal(const PtContext* c, const char* who, int iter_first, int group_iters, float max_fraction, bool folds) {
  if (need(c, who)) return -1;
  return adaptive_refusal(*c, who, iter_first, group_iters, &max_fraction, folds, false);
}
int pt_ctx_enter_adaptive(PtContext* c) {
  if (need(c, "pt_adaptive_round")) return -1;
  HIP_OK(hipSetDevice(c->device));
  return enter_adaptive(*c);
}
int pt_ctx_admit_state(const PtContext* c, const char* who, bool uniform) { return need(c, who) ? -1 : admit(*c, who, kNotFailed | (uniform ? kUniform : 0u)); }

extern "C" {

int pt_ctx_adaptive_round_list(PtContext* c, int iter_first, int group_iters, const int32_t* list_host, int m, int capacity) {
  return round_list_entry(c, "pt_adaptive_round_list", iter_first, group_iters, list_host, true, m, capacity);
}
int pt_ctx_adaptive_round_list_device(PtContext* c, int iter_first, int group_iters, const int32_t* list_dev, int m, int capacity) {
  return round_list_entry(c, "pt_adaptive_round_list", iter_first, group_iters, list_dev, false, m, capacity);
}
const int32_t* pt_ctx_device_counts(PtContext* c) { return c && c->adaptive ? static_cast<const int32_t*>(c->d_acnt) : nullptr; }

int pt_ctx_adaptive_round(PtContext* c, int iter_first, int group_iters, float fraction) {
  if (need(c, "pt_adaptive_round")) return -1;
  Ctx& g = *c;
  if (adaptive_refusal(g, "pt_adaptive_round", iter_first, group_iters, &fraction)) return -1;
  HIP_OK(hipSetDevice(g.device));
  const int W = g.cam.resolution[0];
  if (enter_adaptive(g) || ensure(g, g.d_select, pt_adaptive_select_bytes((size_t)g.N))) return -1;
  const int m = ptad::list_length((double)fraction, g.N);
  if (ensure_worker(g, m)) return -1;  // (a worker of that capacity: its live size is the capacity again, whatever a threshold round left)
  if (pt_adaptive_select_launch(g.stream, W, g.N / W, static_cast<const float*>(g.d_noise), g.d_acnt, m, g.d_select, g.d_list)) return -1;
  return render_and_merge(g, iter_first, group_iters, m);
}

// blend: pt_history_round_threshold, the same round keyed by the variance of the blend
static int round_threshold_entry(PtContext* c, const char* who, bool blend, int iter_first, int group_iters, float threshold, float max_fraction, int* above,
                                 int* selected) {
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (adaptive_refusal(g, who, iter_first, group_iters, &max_fraction)) return -1;
  if (pt_adaptive_check_threshold(who, threshold)) return -1;
  if (blend && history_threshold_refusal(g, who)) return -1;
  return threshold_round(g, who, blend, iter_first, group_iters, threshold, max_fraction, 0, above, selected);
}
int pt_ctx_adaptive_round_threshold(PtContext* c, int iter_first, int group_iters, float threshold, float max_fraction, int* above, int* selected) {
  return round_threshold_entry(c, "pt_adaptive_round_threshold", false, iter_first, group_iters, threshold, max_fraction, above, selected);
}
int pt_ctx_history_round_threshold(PtContext* c, int iter_first, int group_iters, float threshold, float max_fraction, int* above, int* selected) {
  return round_threshold_entry(c, "pt_history_round_threshold", true, iter_first, group_iters, threshold, max_fraction, above, selected);
}

// blend: pt_history_render_threshold, the same driver over rounds keyed by the variance of the blend
static int render_threshold_entry(PtContext* c, const char* who, bool blend, int iter_first, int max_iters, int group_iters, float threshold, float max_fraction,
                                  int min_pixels, int* iters_done, int64_t* samples_done, int* above_left) {
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (max_iters < 1 || (int64_t)iter_first + max_iters - 1 > INT32_MAX || group_iters < 0 || min_pixels < 0)
    return pt_fail("%s: iterations %d, +%d in groups of %d until at most %d pixels are above: the count is >= 1, the group >= 0 (0 = a batch of the worker), the pixels >= 0",
                who, iter_first, max_iters, group_iters, min_pixels);
  // what a round would refuse, apart from the state of the folds, which the uniform groups below establish
  if (adaptive_refusal(g, who, iter_first, group_iters, &max_fraction, false)) return -1;
  if (pt_adaptive_check_threshold(who, threshold)) return -1;
  if (blend && history_threshold_refusal(g, who)) return -1;
  const int cap = ptad::list_length((double)max_fraction, g.N);
  const int group = group_iters ? group_iters : g.worker && g.worker->capacity == cap ? g.worker->K : batch_iters_for(g.opt_iters_per_batch, cap, nullptr);
  int done = 0, above = -1;
  int64_t samples = 0;
  while (done < max_iters) {
    const int n = std::min(group, max_iters - done);
    if (!g.adaptive && g.noise_groups < 2) {  // a uniform group and its fold, as pt_render_adaptive
      if (pt_ctx_render(c, iter_first + done, n) || pt_ctx_noise_fold(c)) return -1;
      samples += (int64_t)n * g.N;
    } else {
      if (!g.adaptive && g.rendered != g.noise_iters && pt_ctx_noise_fold(c)) return -1;  // iterations of the caller's, not yet folded
      if (adaptive_refusal(g, who, iter_first + done, n, &max_fraction)) return -1;
      int m = 0;
      if (threshold_round(g, who, blend, iter_first + done, n, threshold, max_fraction, min_pixels, &above, &m)) return -1;
      if (above <= min_pixels) break;  // nothing was rendered
      samples += (int64_t)n * m;
    }
    done += n;
  }
  if (iters_done) *iters_done = done;
  if (samples_done) *samples_done = samples;
  if (above_left) *above_left = above;
  return 0;
}
int pt_ctx_render_threshold(PtContext* c, int iter_first, int max_iters, int group_iters, float threshold, float max_fraction, int min_pixels,
                            int* iters_done, int64_t* samples_done, int* above_left) {
  return render_threshold_entry(c, "pt_render_threshold", false, iter_first, max_iters, group_iters, threshold, max_fraction, min_pixels, iters_done, samples_done,
                                above_left);
}
int pt_ctx_history_render_threshold(PtContext* c, int iter_first, int max_iters, int group_iters, float threshold, float max_fraction, int min_pixels,
                                    int* iters_done, int64_t* samples_done, int* above_left) {
  return render_threshold_entry(c, "pt_history_render_threshold", true, iter_first, max_iters, group_iters, threshold, max_fraction, min_pixels, iters_done,
                                samples_done, above_left);
}

int pt_ctx_render_adaptive(PtContext* c, int iter_first, int max_iters, int group_iters, float fraction, float target_db, int* iters_done,
                           int64_t* samples_done, float* psnr_db) {
  if (need(c, "pt_render_adaptive")) return -1;
  Ctx& g = *c;
  if (max_iters < 1 || (int64_t)iter_first + max_iters - 1 > INT32_MAX || group_iters < 0 || !std::isfinite(target_db))
    return pt_fail("pt_render_adaptive: iterations %d, +%d in groups of %d until %g dB: the count is >= 1, the group >= 0 (0 = a batch of the worker), the target finite",
                iter_first, max_iters, group_iters, (double)target_db);
  // what a round would refuse, apart from the state of the folds, which the uniform groups below establish
  if (adaptive_refusal(g, "pt_render_adaptive", iter_first, group_iters, &fraction, false)) return -1;
  const int m = ptad::list_length((double)fraction, g.N);
  // group_iters == 0: the iterations per batch a worker for m pixels plans (plan_batches' own function)
  const int group = group_iters ? group_iters : g.worker && g.worker->capacity == m ? g.worker->K : batch_iters_for(g.opt_iters_per_batch, m, nullptr);
  int done = 0;
  int64_t samples = 0;
  float psnr = -1.0f;
  while (done < max_iters) {
    const int n = std::min(group, max_iters - done);
    if (!g.adaptive && g.noise_groups < 2) {  // a uniform group and its fold, as pt_render_until
      if (pt_ctx_render(c, iter_first + done, n) || pt_ctx_noise_fold(c)) return -1;
      samples += (int64_t)n * g.N;
    } else {
      if (!g.adaptive && g.rendered != g.noise_iters && pt_ctx_noise_fold(c)) return -1;  // iterations of the caller's, not yet folded
      if (pt_ctx_adaptive_round(c, iter_first + done, n, fraction)) return -1;
      samples += (int64_t)n * m;
    }
    done += n;
    double sse = -1.0;
    if (pt_ctx_get_noise(c, &sse, nullptr, nullptr)) return -1;
    if (sse < 0.0) continue;  // one group says nothing about the spread
    psnr = pt_psnr_from_sse(sse, g.N);
    if (psnr > target_db) break;
  }
  if (iters_done) *iters_done = done;
  if (samples_done) *samples_done = samples;
  if (psnr_db) *psnr_db = psnr;
  return 0;
}

int pt_ctx_readback_adaptive(PtContext* c, int32_t* counts) {
  if (need(c, "pt_readback_adaptive")) return -1;
  if (!counts) return pt_fail("pt_readback_adaptive: null buffer");
  Ctx& g = *c;
  if (!g.adaptive) {  // the uniform state: the fold's T and M for every pixel
    if (pt_ctx_sync(c)) return -1;
    for (size_t p = 0; p < (size_t)g.N; ++p) counts[2 * p] = (int32_t)std::min<int64_t>(g.noise_iters, INT32_MAX), counts[2 * p + 1] = g.noise_groups;
    return 0;
  }
  static_assert(sizeof(ptad::Cnt) == 2 * sizeof(int32_t), "pt_amd.h: T_p and M_p per pixel");
  return copy_out(c, "pt_readback_adaptive", counts, 2, [&](const int32_t** d) { return *d = static_cast<const int32_t*>(g.d_acnt), 0; });
}

int pt_ctx_resolve_device(PtContext* c, const float** rgb_dev) {
  if (need(c, "pt_resolve")) return -1;
  Ctx& g = *c;
  if (admit(g, "pt_resolve", kNotFailed | kNoExtras)) return -1;
  if (g.noise_groups < 1) return pt_fail("pt_resolve: nothing has been folded (pt_noise_fold): the sample counts are the folds'");
  if (admit(g, "pt_resolve", kFoldedAll)) return -1;
  if (g.noise_iters > INT32_MAX) return pt_fail("pt_resolve: %lld iterations folded", (long long)g.noise_iters);
  HIP_OK(hipSetDevice(g.device));
  if (ensure(g, g.d_resolved, 3 * (size_t)g.N * sizeof(float))) return -1;
  if (pt_adaptive_resolve_launch(g.stream, g.N, g.d_image, g.adaptive ? g.d_acnt : nullptr, (int)g.noise_iters, g.d_resolved)) return -1;
  if (rgb_dev) *rgb_dev = g.d_resolved;
  return 0;
}
int pt_ctx_resolve(PtContext* c, float* rgb_avg_host) {
  return copy_out(c, "pt_resolve", rgb_avg_host, 3, [&](const float** d) { return pt_ctx_resolve_device(c, d); });
}

// ---- reprojected sample history (csrc/pt_history.hip) ---------------------------------------------------------------------
// What the three entry points refuse first, in their order: a failed context, a tile that is not whole rows, the adaptive state.
static int history_admit(const Ctx& g, const char* who) { return admit(g, who, kNotFailed) || admit(g, who, kWholeRows) || admit(g, who, kUniform) ? -1 : 0; }
static pthi::V4* history_plane(const Ctx& g, int plane) { return static_cast<pthi::V4*>(g.d_hist) + (size_t)plane * g.N; }
static const char kNoFeatures[] = "%s: no feature pass has been rendered since the last pt_clear or camera move (pt_render_features)";

static pthi::V4* history_var_plane(const Ctx& g, int plane) { return static_cast<pthi::V4*>(g.d_hist_var) + (size_t)plane * g.N; }  // 0: VK, 1: VC
// An undefined flag bit: what the _ex forms refuse right after a failed context.
// motion: the lookup's word, which also defines PT_HISTORY_MOTION and PT_HISTORY_MATERIALS (alone or beside one of the two).
// PT_HISTORY_FEEDBACK is defined in both words, beside PT_HISTORY_MOMENTS only.
static int history_flags(const char* who, uint32_t flags, bool motion = false) {
  constexpr uint32_t kinds = PT_HISTORY_VARIANCE | PT_HISTORY_MOMENTS;
  const uint32_t defined = kinds | PT_HISTORY_FEEDBACK | (motion ? PT_HISTORY_MOTION | PT_HISTORY_MATERIALS : 0u);
  if (flags & ~defined)
    return pt_fail("%s: undefined flag bit(s) 0x%x (defined: PT_HISTORY_VARIANCE, PT_HISTORY_MOMENTS%s, PT_HISTORY_FEEDBACK)", who, flags & ~defined,
                   motion ? ", PT_HISTORY_MOTION, PT_HISTORY_MATERIALS" : "");
  if ((flags & kinds) == kinds) return pt_fail("%s: the flags PT_HISTORY_VARIANCE and PT_HISTORY_MOMENTS exclude each other", who);
  if ((flags & PT_HISTORY_MATERIALS) && (flags & PT_HISTORY_FEEDBACK))  // (the lookup's word only: the capture's has refused the bit above)
    return pt_fail("%s: PT_HISTORY_MATERIALS is not built beside PT_HISTORY_FEEDBACK: FC carries one variance for three channels, which a per-channel factor cannot scale", who);
  if ((flags & PT_HISTORY_FEEDBACK) && (flags & PT_HISTORY_VARIANCE))
    return pt_fail("%s: PT_HISTORY_FEEDBACK travels beside the moments, not with PT_HISTORY_VARIANCE", who);
  if ((flags & PT_HISTORY_FEEDBACK) && !(flags & PT_HISTORY_MOMENTS))
    return pt_fail("%s: PT_HISTORY_FEEDBACK needs PT_HISTORY_MOMENTS: the filtered colour travels beside the moments", who);
  return 0;
}
static pthi::V4* history_fb_plane(const Ctx& g, int plane) { return static_cast<pthi::V4*>(g.d_hist_fb) + (size_t)plane * g.N; }
// The feedback state: from the first call that carries the flag on
static int history_fb_ensure(Ctx& g) { return ensure(g, g.d_hist_fb, pt_history_feedback_bytes((size_t)g.N), Zero::on_stream); }
// What the variance needs of the folds: at least two, nothing rendered since, and `samples` the iterations they hold.
static int history_folds(const Ctx& g, const char* who, float samples) {
  if (!g.d_noise || g.noise_groups < 1) return pt_fail("%s: nothing has been folded (pt_noise_fold)", who);
  if (g.noise_groups < 2) return pt_fail("%s: %d group(s) folded; a variance needs at least 2 (pt_noise_fold after each group of iterations)", who, g.noise_groups);
  if (admit(g, who, kFoldedAll)) return -1;
  return pt_history_check_fold_samples(who, samples, g.noise_iters);
}
static int history_current_variance(const Ctx& g, const char* who) {
  if (g.hist_current && g.hist_var_current != PT_HISTORY_VARIANCE)
    return pt_fail("%s: the current plane has no variance: the lookup was made without PT_HISTORY_VARIANCE (pt_history_reproject_ex)", who);
  return 0;
}
static int history_current_moments(const Ctx& g, const char* who) {
  if (g.hist_current && g.hist_var_current != PT_HISTORY_MOMENTS)
    return pt_fail("%s: the current plane has no moments: the lookup was made without PT_HISTORY_MOMENTS (pt_history_reproject_ex)", who);
  return 0;
}

// ex: the _ex form, which refuses an undefined flag bit and carries its own name; flags == 0 is the old call either way.
static int history_capture(PtContext* c, const char* who, float samples, uint32_t flags, bool ex) {
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (ex && (admit(g, who, kNotFailed) || history_flags(who, flags))) return -1;
  if (history_admit(g, who)) return -1;
  if (!g.d_feat || !g.feat_fresh) return pt_fail(kNoFeatures, who);
  if (pt_history_check_samples(who, samples)) return -1;
  const bool var = (flags & PT_HISTORY_VARIANCE) != 0, mom = (flags & PT_HISTORY_MOMENTS) != 0, fb = (flags & PT_HISTORY_FEEDBACK) != 0;
  if (var && (admit(g, who, kNoExtras) || history_folds(g, who, samples) || history_current_variance(g, who))) return -1;
  if (mom && history_current_moments(g, who)) return -1;
  if (fb && !g.fb_pending)
    return pt_fail("%s: the pending plane is absent: filter first (pt_history_denoise_feedback after the last pt_render, pt_history_round or pt_render_features)", who);
  HIP_OK(hipSetDevice(g.device));
  if (ensure(g, g.d_hist, pt_history_state_bytes((size_t)g.N), Zero::on_stream)) return -1;  // the first capture of the context
  if ((var || mom) && ensure(g, g.d_hist_var, pt_history_variance_bytes((size_t)g.N), Zero::on_stream)) return -1;  // ... with variance or moments
  const pthi::V4* current = g.hist_current ? history_plane(g, pthi::kKeptPlanes) : nullptr;
  if (var) {
    const ptnz::Fold f = ptnz::fold_scalars(1, g.noise_groups, g.noise_iters);
    if (pt_history_capture_variance_launch(g.stream, g.N, g.d_image, reinterpret_cast<const float*>(g.d_feat), current, samples, g.d_hist,
                                           static_cast<const float*>(g.d_noise), f.Tf, f.Df, current ? history_var_plane(g, 1) : nullptr, history_var_plane(g, 0)))
      return -1;
  } else if (mom) {
    if (g.hist_extra ? pt_history_capture_moments_counted_launch(g.stream, g.N, g.d_image, reinterpret_cast<const float*>(g.d_feat), current, samples,
                                                                 g.d_hist_extra, g.d_hist, current ? history_var_plane(g, 1) : nullptr, history_var_plane(g, 0))
                     : pt_history_capture_moments_launch(g.stream, g.N, g.d_image, reinterpret_cast<const float*>(g.d_feat), current, samples, g.d_hist,
                                                         current ? history_var_plane(g, 1) : nullptr, history_var_plane(g, 0)))
      return -1;
  } else if (g.hist_extra) {  // counted: ns = samples + E_p
    if (pt_history_capture_counted_launch(g.stream, g.N, g.d_image, reinterpret_cast<const float*>(g.d_feat), current, samples, g.d_hist_extra, g.d_hist)) return -1;
  } else if (pt_history_capture_launch(g.stream, g.N, g.d_image, reinterpret_cast<const float*>(g.d_feat), current, samples, g.d_hist)) {
    return -1;
  }
  g.hist_cam = g.cam;
  if (PtHistoryMotion& hm = g.hist_motion; hm.geoms_stale) hm.geoms = g.camera_base.geoms, hm.geoms_stale = false, hm.fresh = false;  // the kept geoms: retaken only after a pt_set_geoms
  if (PtHistoryMaterials& hm = g.hist_materials; hm.stale) hm.materials = g.materials, hm.stale = false, hm.fresh = false;  // the kept materials: retaken only after a pt_set_materials
  g.hist_kept = true;
  g.hist_var_kept = flags & ~PT_HISTORY_FEEDBACK;  // a plain capture: kept without variance or moments
  if (fb) std::swap(g.fb_plane_kept, g.fb_plane_pending), g.fb_pending = false;  // FK := P: the roles change, no bytes move
  g.fb_kept = fb;  // a capture without the flag: kept without feedback
  return 0;
}
int pt_ctx_history_capture(PtContext* c, float samples) { return history_capture(c, "pt_history_capture", samples, 0u, false); }
int pt_ctx_history_capture_ex(PtContext* c, float samples, uint32_t flags) { return history_capture(c, "pt_history_capture_ex", samples, flags, true); }

// A per-geom table of pt_amd.h, one byte per geom: 1 where `field` of the geom's material is positive (reject_geom: reflective;
// emitter_geom: emittance), from the tables the renderer holds on the host — the geoms' material ids and the materials.  Blocking;
// once per context and table, and once more after every pt_ctx_set_materials (stale; that call synchronised, and nothing has read the
// table since, so it is written in place).
static int history_geom_table(Ctx& g, uint8_t*& d_table, bool& stale, float ptd::Mat::*field) {
  if (d_table && !stale) return 0;
  const std::vector<ptd::Mat> mats = pt::material_table(g.materials.data(), (int)g.materials.size());  // what the device table holds
  const std::vector<PtGeom>& geoms = g.camera_base.geoms;
  std::vector<uint8_t> table(std::max<size_t>(geoms.size(), 1), 0);
  for (size_t i = 0; i < geoms.size(); ++i) {
    const int32_t m = geoms[i].materialid;
    table[i] = m >= 0 && (size_t)m < mats.size() && mats[(size_t)m].*field > 0.0f ? 1 : 0;
  }
  if (ensure(g, d_table, table.size())) return -1;
  HIP_OK(hipMemcpy(d_table, table.data(), table.size(), hipMemcpyHostToDevice));
  stale = false;
  return 0;
}
static int history_reject_table(Ctx& g) { return history_geom_table(g, g.d_hist_reject, g.hist_reject_stale, &ptd::Mat::reflective); }

// The motion table of the kept geoms of `hm` and the current geoms (pthi::motion_table) on g's device, for a lookup with
// PT_HISTORY_MOTION; hm: the context's own, or the one a group keeps for the frame's K (then g is the group's root context).
// *moved == false: every geom is still; nothing was allocated or uploaded and the caller launches the kernel without the flag.
// The table follows from the kept and the current geoms alone, so it is computed by the first lookup after either changed (a capture
// that retook the geoms, pt_ctx_set_geoms) and uploaded when it differs from what the device holds (synchronises then: the staging
// is pageable); later lookups find it in place — on 10,170 geoms the host's 0.3 ms per call would otherwise be nine times the kernel.
static int history_motion_table(Ctx& g, PtHistoryMotion& hm, bool* moved) {
  const std::vector<PtGeom>& cur = g.camera_base.geoms;
  const size_t n = cur.size();
  *moved = false;
  if (hm.geoms.size() != n || n == 0) return 0;  // (nothing kept yet: the caller has refused already)
  if (hm.fresh) return *moved = hm.moved, 0;
  std::vector<float> table(n * pthi::kMotionRow);
  std::vector<uint8_t> kind(n);
  pthi::motion_table(hm.geoms.data(), cur.data(), (int)n, table.data(), kind.data());
  for (uint8_t k : kind) *moved = *moved || k != pthi::kStill;
  hm.moved = *moved;
  if (!*moved) return hm.fresh = true, 0;
  const size_t table_bytes = table.size() * sizeof(float);
  if (ensure(g, hm.d_table, table_bytes + n)) return -1;
  if (table != hm.table || kind != hm.kind) {
    HIP_OK(hipStreamSynchronize(g.stream));  // an earlier lookup may still read the rows
    HIP_OK(hipMemcpy(hm.d_table, table.data(), table_bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(static_cast<char*>(hm.d_table) + table_bytes, kind.data(), n, hipMemcpyHostToDevice));
    hm.table = std::move(table), hm.kind = std::move(kind);
  }
  hm.fresh = true;
  return 0;
}

// The recolour table of the kept materials of `hm` and the current ones (pthi::recolor_table) on g's device, for a lookup with
// PT_HISTORY_MATERIALS, as history_motion_table: *edited == false: every material is what it was at the capture; nothing was allocated
// or uploaded and the caller launches the kernel of the same call without the flag.  Computed by the first lookup after a capture
// that retook the materials or a pt_ctx_set_materials, uploaded when it differs from what the device holds (synchronises then).
static int history_recolor_table(Ctx& g, PtHistoryMaterials& hm, bool* edited) {
  const std::vector<PtGeom>& geoms = g.camera_base.geoms;
  const size_t n = geoms.size();
  *edited = false;
  if (hm.materials.size() != g.materials.size() || n == 0) return 0;  // (nothing kept yet: the caller has refused already — every capture keeps the materials)
  if (hm.fresh) return *edited = hm.changed, 0;
  std::vector<float> table(n * pthi::kRecolorRow);
  std::vector<uint8_t> kind(n);
  pthi::recolor_table(hm.materials.data(), g.materials.data(), (int)g.materials.size(), geoms.data(), (int)n, table.data(), kind.data());
  for (uint8_t k : kind) *edited = *edited || k != pthi::kUnchanged;
  hm.changed = *edited;
  if (!*edited) return hm.fresh = true, 0;
  const size_t table_bytes = table.size() * sizeof(float);
  if (ensure(g, hm.d_table, table_bytes + n)) return -1;
  if (table != hm.table || kind != hm.kind) {
    HIP_OK(hipStreamSynchronize(g.stream));  // an earlier lookup may still read the rows
    HIP_OK(hipMemcpy(hm.d_table, table.data(), table_bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(static_cast<char*>(hm.d_table) + table_bytes, kind.data(), n, hipMemcpyHostToDevice));
    hm.table = std::move(table), hm.kind = std::move(kind);
  }
  hm.fresh = true;
  return 0;
}

static int history_reproject(PtContext* c, const char* who, const PtHistoryOptions* opt, uint32_t flags, bool ex) {
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (ex && (admit(g, who, kNotFailed) || history_flags(who, flags, true))) return -1;
  const bool motion = (flags & PT_HISTORY_MOTION) != 0, fb = (flags & PT_HISTORY_FEEDBACK) != 0, materials = (flags & PT_HISTORY_MATERIALS) != 0;
  flags &= ~(PT_HISTORY_MOTION | PT_HISTORY_FEEDBACK | PT_HISTORY_MATERIALS);  // what is left names the kind: 0, PT_HISTORY_VARIANCE or PT_HISTORY_MOMENTS
  if (history_admit(g, who)) return -1;
  if (!g.d_hist || !g.hist_kept) return pt_fail("%s: nothing has been captured (pt_history_capture)", who);
  if (!g.d_feat || !g.feat_fresh) return pt_fail(kNoFeatures, who);
  pthi::Params P{};
  if (pt_history_resolve_options(who, opt, &P)) return -1;
  if (flags == PT_HISTORY_VARIANCE && (!g.d_hist_var || g.hist_var_kept != PT_HISTORY_VARIANCE))
    return pt_fail("%s: nothing has been captured with variance (pt_history_capture_ex with PT_HISTORY_VARIANCE)", who);
  if (flags == PT_HISTORY_MOMENTS && (!g.d_hist_var || g.hist_var_kept != PT_HISTORY_MOMENTS))
    return pt_fail("%s: nothing has been captured with moments (pt_history_capture_ex with PT_HISTORY_MOMENTS)", who);
  if (fb && (!g.d_hist_fb || !g.fb_kept))
    return pt_fail("%s: nothing has been captured with feedback (pt_history_capture_ex with PT_HISTORY_MOMENTS | PT_HISTORY_FEEDBACK)", who);
  HIP_OK(hipSetDevice(g.device));
  if (history_reject_table(g)) return -1;
  const int W = g.cam.resolution[0];
  const pthi::View v = pthi::make_view(g.hist_cam, g.N / W, g.pixel_begin / W);
  const float* feat = reinterpret_cast<const float*>(g.d_feat);
  const int num_geoms = (int)g.camera_base.geoms.size();
  bool moved = false;
  if (motion && history_motion_table(g, g.hist_motion, &moved)) return -1;
  bool edited = false;
  if (materials && history_recolor_table(g, g.hist_materials, &edited)) return -1;
  if (edited) {  // (never beside fb: the flag word refused that)
    const float* table = moved ? static_cast<const float*>(g.hist_motion.d_table) : nullptr;
    const uint8_t* kind = moved ? reinterpret_cast<const uint8_t*>(table + (size_t)num_geoms * pthi::kMotionRow) : nullptr;
    const float* recolor = static_cast<const float*>(g.hist_materials.d_table);
    const uint8_t* rkind = reinterpret_cast<const uint8_t*>(recolor + (size_t)num_geoms * pthi::kRecolorRow);
    if (pt_history_reproject_materials_launch(g.stream, flags, v, g.d_hist, feat, g.d_hist_reject, num_geoms, P, history_plane(g, pthi::kKeptPlanes),
                                              flags ? history_var_plane(g, 0) : nullptr, flags ? history_var_plane(g, 1) : nullptr, table, kind, recolor, rkind))
      return -1;
  } else if (fb) {
    const float* table = moved ? static_cast<const float*>(g.hist_motion.d_table) : nullptr;
    const uint8_t* kind = moved ? reinterpret_cast<const uint8_t*>(table + (size_t)num_geoms * pthi::kMotionRow) : nullptr;
    if (pt_history_reproject_feedback_launch(g.stream, v, g.d_hist, feat, g.d_hist_reject, num_geoms, P, history_plane(g, pthi::kKeptPlanes), history_var_plane(g, 0),
                                             history_var_plane(g, 1), history_fb_plane(g, g.fb_plane_kept), history_fb_plane(g, g.fb_plane_current), table, kind))
      return -1;
  } else if (moved) {
    const float* table = static_cast<const float*>(g.hist_motion.d_table);
    const uint8_t* kind = reinterpret_cast<const uint8_t*>(table + (size_t)num_geoms * pthi::kMotionRow);
    if (pt_history_reproject_motion_launch(g.stream, flags, v, g.d_hist, feat, g.d_hist_reject, num_geoms, P, history_plane(g, pthi::kKeptPlanes),
                                           flags ? history_var_plane(g, 0) : nullptr, flags ? history_var_plane(g, 1) : nullptr, table, kind))
      return -1;
  } else if (flags == PT_HISTORY_VARIANCE
          ? pt_history_reproject_variance_launch(g.stream, v, g.d_hist, feat, g.d_hist_reject, num_geoms, P, history_plane(g, pthi::kKeptPlanes),
                                                 history_var_plane(g, 0), history_var_plane(g, 1))
      : flags == PT_HISTORY_MOMENTS
          ? pt_history_reproject_moments_launch(g.stream, v, g.d_hist, feat, g.d_hist_reject, num_geoms, P, history_plane(g, pthi::kKeptPlanes),
                                                history_var_plane(g, 0), history_var_plane(g, 1))
          : pt_history_reproject_launch(g.stream, v, g.d_hist, feat, g.d_hist_reject, num_geoms, P, history_plane(g, pthi::kKeptPlanes)))
    return -1;
  g.hist_current = true;
  g.hist_var_current = flags;
  g.fb_current = fb;  // a lookup without the flag leaves FC absent
  g.probe_applied = false;  // a new C: the probes may be checked against it
  return 0;
}
int pt_ctx_history_reproject(PtContext* c, const PtHistoryOptions* opt) { return history_reproject(c, "pt_history_reproject", opt, 0u, false); }
int pt_ctx_history_reproject_ex(PtContext* c, const PtHistoryOptions* opt, uint32_t flags) {
  return history_reproject(c, "pt_history_reproject_ex", opt, flags, true);
}

// ---- the guided filter over the blend (ptdn::Form::History) --------------------------------------------------------------
// Everything pt_history_denoise refuses but the null buffer, in its order; the job resolved.
static int history_denoise_refusal(const Ctx& g, const char* who, float samples, const PtDenoiseOptions* opt, ptdn::Job* j) {
  if (history_admit(g, who) || admit(g, who, kNoExtras)) return -1;  // (the fold's variance knows nothing of the extras)
  if (!g.d_feat || !g.feat_fresh) return pt_fail(kNoFeatures, who);
  if (pt_history_check_samples(who, samples)) return -1;
  ptdn::Params P{};
  if (const char* msg = ptdn::resolve(opt, &P, ptdn::kHistorySigmaColor)) return pt_fail("%s: %s", who, msg);
  if (history_folds(g, who, samples) || history_current_variance(g, who)) return -1;
  return pt_denoise_resolve(who, ptdn::Form::History, samples, g.noise_groups, g.noise_iters, opt, j);
}
static int history_denoise_device(PtContext* c, const char* who, float samples, const PtDenoiseOptions* opt, const float** rgb_dev) {
  if (need(c, who)) return -1;
  Ctx& g = *c;
  ptdn::Job j{};
  if (history_denoise_refusal(g, who, samples, opt, &j)) return -1;
  if (!rgb_dev) return pt_fail("%s: null buffer", who);
  HIP_OK(hipSetDevice(g.device));
  if (ensure(g, g.d_denoise, pt_denoise_workspace_bytes((size_t)g.N))) return -1;  // the first denoise call of the context, of any kind
  const int W = g.cam.resolution[0];
  j.f = {W, g.N / W, g.d_image, reinterpret_cast<const float*>(g.d_feat), static_cast<const float*>(g.d_noise)};
  if (g.hist_current) {
    j.div.C = reinterpret_cast<const ptdn::V4*>(history_plane(g, pthi::kKeptPlanes));
    j.div.VC = reinterpret_cast<const ptdn::V4*>(history_var_plane(g, 1));
  }
  return pt_denoise_launch(g.stream, j, g.d_denoise, rgb_dev);
}
int pt_ctx_history_denoise_device(PtContext* c, float samples, const PtDenoiseOptions* opt, const float** rgb_dev) {
  return history_denoise_device(c, "pt_history_denoise", samples, opt, rgb_dev);
}
int pt_ctx_history_denoise(PtContext* c, float samples, const PtDenoiseOptions* opt, float* rgb_avg_host) {
  if (need(c, "pt_history_denoise")) return -1;
  ptdn::Job j{};
  if (history_denoise_refusal(*c, "pt_history_denoise", samples, opt, &j)) return -1;  // (before the null buffer)
  return copy_out(c, "pt_history_denoise", rgb_avg_host, 3, [&](const float** d) { return pt_ctx_history_denoise_device(c, samples, opt, d); });
}

// ---- ... and with the history's moments (ptdn::Form::Moments) -----------------------------------------------------------------
// Everything pt_history_denoise_ex refuses with PT_HISTORY_MOMENTS but the null buffer, in its order (the flag word: the callers); the
// job resolved.  No fold conditions: the form reads no noise planes.
static int history_denoise_moments_refusal(const Ctx& g, const char* who, float samples, const PtDenoiseOptions* opt, ptdn::Job* j) {
  if (history_admit(g, who)) return -1;
  if (!g.d_feat || !g.feat_fresh) return pt_fail(kNoFeatures, who);
  if (pt_history_check_samples(who, samples)) return -1;
  if (pt_denoise_resolve(who, ptdn::Form::Moments, samples, 0, 0, opt, j)) return -1;
  return history_current_moments(g, who);
}
// The flag word of pt_history_denoise_ex: PT_HISTORY_MOMENTS or nothing.
static int history_denoise_flags(const char* who, uint32_t flags) {
  if (flags & ~PT_HISTORY_MOMENTS) return pt_fail("%s: undefined flag bit(s) 0x%x (defined: PT_HISTORY_MOMENTS)", who, flags & ~PT_HISTORY_MOMENTS);
  return 0;
}
int pt_ctx_history_denoise_ex_device(PtContext* c, float samples, const PtDenoiseOptions* opt, uint32_t flags, const float** rgb_dev) {
  const char* who = "pt_history_denoise_ex";
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (admit(g, who, kNotFailed) || history_denoise_flags(who, flags)) return -1;
  if (!flags) return history_denoise_device(c, who, samples, opt, rgb_dev);
  ptdn::Job j{};
  if (history_denoise_moments_refusal(g, who, samples, opt, &j)) return -1;
  if (!rgb_dev) return pt_fail("%s: null buffer", who);
  HIP_OK(hipSetDevice(g.device));
  if (ensure(g, g.d_denoise, pt_denoise_workspace_bytes((size_t)g.N))) return -1;  // the first denoise call of the context, of any kind
  const int W = g.cam.resolution[0];
  j.f = {W, g.N / W, g.d_image, reinterpret_cast<const float*>(g.d_feat), nullptr};
  if (g.hist_current) {
    j.div.C = reinterpret_cast<const ptdn::V4*>(history_plane(g, pthi::kKeptPlanes));
    j.div.VC = reinterpret_cast<const ptdn::V4*>(history_var_plane(g, 1));
  }
  j.div.E = g.hist_extra ? g.d_hist_extra : nullptr;  // counted: the prepare reads ns = samples + E_p
  return pt_denoise_launch(g.stream, j, g.d_denoise, rgb_dev);
}
int pt_ctx_history_denoise_ex(PtContext* c, float samples, const PtDenoiseOptions* opt, uint32_t flags, float* rgb_avg_host) {
  const char* who = "pt_history_denoise_ex";
  if (need(c, who)) return -1;
  if (admit(*c, who, kNotFailed) || history_denoise_flags(who, flags)) return -1;
  ptdn::Job j{};
  if (flags ? history_denoise_moments_refusal(*c, who, samples, opt, &j) : history_denoise_refusal(*c, who, samples, opt, &j)) return -1;  // (before the null buffer)
  return copy_out(c, who, rgb_avg_host, 3, [&](const float** d) { return pt_ctx_history_denoise_ex_device(c, samples, opt, flags, d); });
}

// ---- ... and with the filtered history (ptdn::Form::Feedback) ----------------------------------------------------------------
// Everything pt_history_denoise_feedback refuses but the null buffer, in its order: the moments form's, then fb out of range, C without
// FC, and rule 1 in another unit than the one FC.w was tapped in; the job resolved.
static int history_denoise_feedback_refusal(const Ctx& g, const char* who, float samples, const PtDenoiseOptions* opt, const PtHistoryFeedbackOptions* fb,
                                            ptdn::Job* j) {
  if (history_denoise_moments_refusal(g, who, samples, opt, j)) return -1;
  j->form = ptdn::Form::Feedback;
  if (pt_history_feedback_options(who, fb, j->P.levels, &j->tap_level, &j->div.fb_variance)) return -1;
  if (g.hist_current && !g.fb_current)
    return pt_fail("%s: the current plane has no filtered colour: the lookup was made without PT_HISTORY_FEEDBACK (pt_history_reproject_ex)", who);
  if (j->div.fb_variance == 1 && g.fb_current && j->P.keep_albedo != g.fb_keep_albedo)
    return pt_fail("%s: feedback variance 1 with keep_albedo %d, but the carried variance was tapped with keep_albedo %d: the two are in different units", who,
                   j->P.keep_albedo, g.fb_keep_albedo);
  return 0;
}
int pt_ctx_history_denoise_feedback_device(PtContext* c, float samples, const PtDenoiseOptions* opt, const PtHistoryFeedbackOptions* fb, const float** rgb_dev) {
  const char* who = "pt_history_denoise_feedback";
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (admit(g, who, kNotFailed)) return -1;
  ptdn::Job j{};
  if (history_denoise_feedback_refusal(g, who, samples, opt, fb, &j)) return -1;
  if (!rgb_dev) return pt_fail("%s: null buffer", who);
  HIP_OK(hipSetDevice(g.device));
  if (ensure(g, g.d_denoise, pt_denoise_workspace_bytes((size_t)g.N)) || history_fb_ensure(g)) return -1;
  const int W = g.cam.resolution[0];
  j.f = {W, g.N / W, g.d_image, reinterpret_cast<const float*>(g.d_feat), nullptr};
  if (g.hist_current) {
    j.div.C = reinterpret_cast<const ptdn::V4*>(history_plane(g, pthi::kKeptPlanes));
    j.div.VC = reinterpret_cast<const ptdn::V4*>(history_var_plane(g, 1));
    j.div.FC = reinterpret_cast<const ptdn::V4*>(history_fb_plane(g, g.fb_plane_current));
  }
  j.div.E = g.hist_extra ? g.d_hist_extra : nullptr;  // counted: the prepare reads ns = samples + E_p
  j.tap = history_fb_plane(g, g.fb_plane_pending);
  g.fb_pending = false;
  if (pt_denoise_launch(g.stream, j, g.d_denoise, rgb_dev)) return -1;
  g.fb_pending = true;
  g.fb_keep_albedo = j.P.keep_albedo;
  return 0;
}
int pt_ctx_history_denoise_feedback(PtContext* c, float samples, const PtDenoiseOptions* opt, const PtHistoryFeedbackOptions* fb, float* rgb_avg_host) {
  const char* who = "pt_history_denoise_feedback";
  if (need(c, who)) return -1;
  if (admit(*c, who, kNotFailed)) return -1;
  ptdn::Job j{};
  if (history_denoise_feedback_refusal(*c, who, samples, opt, fb, &j)) return -1;  // (before the null buffer)
  return copy_out(c, who, rgb_avg_host, 3, [&](const float** d) { return pt_ctx_history_denoise_feedback_device(c, samples, opt, fb, d); });
}

// FK, FC and P, each N float4; an absent plane reads as zeros; any pointer may be NULL
int pt_ctx_readback_history_feedback(PtContext* c, float* kept, float* current, float* pending) {
  if (need(c, "pt_readback_history_feedback")) return -1;
  Ctx& g = *c;
  HIP_OK(hipSetDevice(g.device));
  const size_t plane = (size_t)g.N * sizeof(pthi::V4);
  float* const host[3] = {kept, current, pending};
  const bool have[3] = {g.d_hist_fb && g.fb_kept, g.d_hist_fb && g.fb_current, g.d_hist_fb && g.fb_pending};
  const int at[3] = {g.fb_plane_kept, g.fb_plane_current, g.fb_plane_pending};
  for (int k = 0; k < 3; ++k)
    if (host[k] && have[k]) HIP_OK(hipMemcpyAsync(host[k], history_fb_plane(g, at[k]), plane, hipMemcpyDeviceToHost, g.stream));
  if (pt_ctx_sync(c)) return -1;
  for (int k = 0; k < 3; ++k)
    if (host[k] && !have[k]) std::fill(host[k], host[k] + 4 * (size_t)g.N, 0.0f);
  return 0;
}

int pt_ctx_history_resolve_device(PtContext* c, float samples, const float** rgb_dev) {
  if (need(c, "pt_history_resolve")) return -1;
  Ctx& g = *c;
  if (history_admit(g, "pt_history_resolve")) return -1;
  if (pt_history_check_samples("pt_history_resolve", samples)) return -1;
  if (!rgb_dev) return pt_fail("pt_history_resolve: null buffer");
  HIP_OK(hipSetDevice(g.device));
  if (ensure(g, g.d_resolved, 3 * (size_t)g.N * sizeof(float))) return -1;
  const pthi::V4* current = g.hist_current ? history_plane(g, pthi::kKeptPlanes) : nullptr;
  if (g.hist_extra ? pt_history_blend_counted_launch(g.stream, g.N, g.d_image, samples, g.d_hist_extra, current, g.d_resolved)
                   : pt_history_blend_launch(g.stream, g.N, g.d_image, samples, current, g.d_resolved))
    return -1;
  *rgb_dev = g.d_resolved;
  return 0;
}
int pt_ctx_history_resolve(PtContext* c, float samples, float* rgb_avg_host) {
  if (need(c, "pt_history_resolve")) return -1;
  if (history_admit(*c, "pt_history_resolve") || pt_history_check_samples("pt_history_resolve", samples)) return -1;  // (before the null buffer)
  return copy_out(c, "pt_history_resolve", rgb_avg_host, 3, [&](const float** d) { return pt_ctx_history_resolve_device(c, samples, d); });
}

int pt_ctx_readback_history(PtContext* c, float* kept_planes, float* current_plane) {
  if (need(c, "pt_readback_history")) return -1;
  Ctx& g = *c;
  if (!g.d_hist) return pt_fail("pt_readback_history: nothing has been captured (pt_history_capture)");
  HIP_OK(hipSetDevice(g.device));
  const size_t plane = (size_t)g.N * sizeof(pthi::V4);
  if (kept_planes) HIP_OK(hipMemcpyAsync(kept_planes, g.d_hist, pthi::kKeptPlanes * plane, hipMemcpyDeviceToHost, g.stream));
  if (current_plane && g.hist_current) HIP_OK(hipMemcpyAsync(current_plane, history_plane(g, pthi::kKeptPlanes), plane, hipMemcpyDeviceToHost, g.stream));
  if (pt_ctx_sync(c)) return -1;
  if (current_plane && !g.hist_current) std::fill(current_plane, current_plane + 4 * (size_t)g.N, 0.0f);
  return 0;
}

int pt_ctx_readback_history_variance(PtContext* c, float* kept_var, float* current_var) {
  if (need(c, "pt_readback_history_variance")) return -1;
  Ctx& g = *c;
  HIP_OK(hipSetDevice(g.device));
  const size_t plane = (size_t)g.N * sizeof(pthi::V4);
  const bool kept = g.d_hist_var && g.hist_var_kept, current = g.d_hist_var && g.hist_var_current;  // (whichever kind they hold)
  if (kept_var && kept) HIP_OK(hipMemcpyAsync(kept_var, history_var_plane(g, 0), plane, hipMemcpyDeviceToHost, g.stream));
  if (current_var && current) HIP_OK(hipMemcpyAsync(current_var, history_var_plane(g, 1), plane, hipMemcpyDeviceToHost, g.stream));
  if (pt_ctx_sync(c)) return -1;
  if (kept_var && !kept) std::fill(kept_var, kept_var + 4 * (size_t)g.N, 0.0f);
  if (current_var && !current) std::fill(current_var, current_var + 4 * (size_t)g.N, 0.0f);
  return 0;
}

// ---- the history round: a group of further iterations for the pixels whose history is short --------------------------------
// emitter_geom of pt_amd.h, as history_reject_table.
static int history_emitter_table(Ctx& g) { return history_geom_table(g, g.d_hist_emitter, g.hist_emitter_stale, &ptd::Mat::emittance); }

// What the round and the round over a caller's list refuse first: a failed context, the iteration range, the convergence metric.
static int history_round_head(const Ctx& g, const char* who, int iter_first, int group_iters) {
  if (admit(g, who, kNotFailed)) return -1;
  if (iter_first < 1 || group_iters < 1 || (int64_t)iter_first + group_iters - 1 > INT32_MAX)
    return pt_fail("%s: iterations %d, +%d: the first is >= 1, the group holds at least one", who, iter_first, group_iters);
  if (g.conv) return pt_fail("%s: the renderer was created with PtOptions.convergence = %d; the convergence metric follows whole iterations", who, g.conv);
  return 0;
}
// Everything pt_history_round refuses before its options; rows == false: apart from the tile's rows (a group's context).
static int history_round_refusal(const Ctx& g, const char* who, int iter_first, int group_iters, bool rows) {
  if (history_round_head(g, who, iter_first, group_iters)) return -1;
  if ((rows && admit(g, who, kWholeRows)) || admit(g, who, kUniform)) return -1;
  if (!g.d_feat || !g.feat_fresh) return pt_fail(kNoFeatures, who);
  return 0;
}

// The second half of a round, after key and selection: the m >= 0 pixels of g.d_list on the worker's live tile, merged into the image
// and E.  E is ensured (zeroed) and made present even for m == 0, so that the contexts of a group agree on whether it exists.
static int history_render_and_merge(Ctx& g, int iter_first, int group_iters, int m) {
  if (ensure(g, g.d_hist_extra, (size_t)g.N * sizeof(float), Zero::on_stream)) return -1;  // the first round that renders (pt_clear zeroes it from then on)
  g.hist_extra = true;
  if (m == 0) return 0;
  set_worker_live(*g.worker, m);
  if (render_list(g, iter_first, group_iters)) return -1;
  if (pt_history_merge_launch(g.stream, g.N, g.d_image, g.d_hist_extra, g.d_list, m, g.worker->d_image, group_iters)) return -1;
  g.samples += (int64_t)group_iters * m;
  return 0;
}

// pt_history_round_list: to pt_history_round what pt_adaptive_round_list is to the threshold round — the round without key and
// selection, over a caller's list of tile pixels; allowed on a striped tile (it reads no features and no C, and needs no whole rows).
// `list` on the host or on the context's device, as in round_list().
static int history_round_list(PtContext* c, const char* who, int iter_first, int group_iters, const int32_t* list, bool host, int m, int capacity) {
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (history_round_head(g, who, iter_first, group_iters) || admit(g, who, kUniform)) return -1;
  if (capacity < 1 || capacity > g.N || m < 0 || m > capacity)
    return pt_fail("%s: a list of %d on a worker for %d out of %d pixels: the capacity is 1 .. the tile, the list 0 .. the capacity", who, m, capacity, g.N);
  if (m > 0 && !list) return pt_fail("%s: null list", who);
  for (int i = 0; host && i < m; ++i)
    if (list[i] < 0 || list[i] >= g.N || (i > 0 && list[i] <= list[i - 1]))
      return pt_fail("%s: list[%d] = %d is outside the tile or not above its predecessor", who, i, list[i]);
  HIP_OK(hipSetDevice(g.device));
  if (ensure_worker(g, capacity)) return -1;
  if (m > 0) {
    HIP_OK(hipMemcpyAsync(g.d_list, list, (size_t)m * sizeof(int32_t), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, g.stream));
    if (g.stripe && pt_group_offsets_launch(g.stream, g.d_list, m, g.stripe, g.stripe_stride - g.stripe, g.d_list_frame)) return -1;
  }
  g.fb_pending = false;  // as in pt_history_round: the pending plane is the filter of the image before the round
  return history_render_and_merge(g, iter_first, group_iters, m);
}

}  // extern "C"
// pt_context.h: what a group's history asks of its contexts
int pt_ctx_admit_no_extras(const PtContext* c, const char* who) { return need(c, who) ? -1 : admit(*c, who, kNoExtras); }
bool pt_ctx_features_fresh(const PtContext* c) { return c && c->d_feat && c->feat_fresh; }
bool pt_ctx_history_extra_present(const PtContext* c) { return c && c->hist_extra; }
const float* pt_ctx_device_history_extra(PtContext* c) { return c && c->hist_extra ? c->d_hist_extra : nullptr; }
int pt_history_check_flags(const char* who, uint32_t flags, bool motion) { return history_flags(who, flags, motion); }
int pt_history_check_denoise_flags(const char* who, uint32_t flags) { return history_denoise_flags(who, flags); }
int pt_ctx_history_round_refusal(const PtContext* c, const char* who, int iter_first, int group_iters) {
  return need(c, who) ? -1 : history_round_refusal(*c, who, iter_first, group_iters, false);
}
int pt_ctx_history_geom_table(PtContext* c, bool emitter, const uint8_t** table_dev, int* num_geoms) {
  if (need(c, "pt_group_history")) return -1;
  Ctx& g = *c;
  HIP_OK(hipSetDevice(g.device));
  if (emitter ? history_emitter_table(g) : history_reject_table(g)) return -1;
  *table_dev = emitter ? g.d_hist_emitter : g.d_hist_reject;
  *num_geoms = (int)g.camera_base.geoms.size();
  return 0;
}
int pt_ctx_history_motion_table(PtContext* c, PtHistoryMotion* m, const float** table_dev, const uint8_t** kind_dev) {
  if (need(c, "pt_group_history")) return -1;
  Ctx& g = *c;
  HIP_OK(hipSetDevice(g.device));
  bool moved = false;
  if (history_motion_table(g, *m, &moved)) return -1;
  *table_dev = moved ? static_cast<const float*>(m->d_table) : nullptr;
  *kind_dev = moved ? reinterpret_cast<const uint8_t*>(*table_dev + g.camera_base.geoms.size() * pthi::kMotionRow) : nullptr;
  return 0;
}
const std::vector<PtGeom>& pt_ctx_geoms(const PtContext* c) { return c->camera_base.geoms; }
const PtCamera& pt_ctx_camera(const PtContext* c) { return c->cam; }
extern "C" {

int pt_ctx_history_round_list(PtContext* c, int iter_first, int group_iters, const int32_t* list_host, int m, int capacity) {
  return history_round_list(c, "pt_history_round_list", iter_first, group_iters, list_host, true, m, capacity);
}
int pt_ctx_history_round_list_device(PtContext* c, int iter_first, int group_iters, const int32_t* list_dev, int m, int capacity) {
  return history_round_list(c, "pt_history_round_list", iter_first, group_iters, list_dev, false, m, capacity);
}

int pt_ctx_history_round(PtContext* c, int iter_first, int group_iters, const PtHistoryRoundOptions* opt, int* fresh, int* selected) {
  const char* who = "pt_history_round";
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (history_round_refusal(g, who, iter_first, group_iters, true)) return -1;
  pthi::RoundParams P{};
  if (pt_history_round_options(who, opt, &P)) return -1;
  HIP_OK(hipSetDevice(g.device));
  const int W = g.cam.resolution[0];
  const int cap = ptad::list_length((double)P.max_fraction, g.N);
  if (history_emitter_table(g) || ensure(g, g.d_select, pt_adaptive_select_bytes((size_t)g.N)) || ensure_worker(g, cap)) return -1;
  // key and select; the two counts read back (8 bytes and ONE synchronise: the list's length decides the launches that follow)
  if (pt_history_key_launch(g.stream, g.N, reinterpret_cast<const float*>(g.d_feat), g.hist_current ? history_plane(g, pthi::kKeptPlanes) : nullptr,
                            g.d_hist_emitter, (int)g.camera_base.geoms.size(), P.min_history, pt_adaptive_select_keys(g.d_select, (size_t)g.N)))
    return -1;
  if (pt_adaptive_select_threshold_keys_launch(g.stream, W, g.N / W, 0.0f, cap, g.d_select, g.d_list)) return -1;
  uint32_t result[2] = {0u, 0u};  // fresh, m
  HIP_OK(hipMemcpyAsync(result, pt_adaptive_select_result(g.d_select, (size_t)g.N), sizeof(result), hipMemcpyDeviceToHost, g.stream));
  HIP_OK(hipStreamSynchronize(g.stream));
  const int m = (int)result[1];
  if (m < 0 || m > cap || (int)result[0] < m) return pt_fail("%s: the selection left %u fresh, a list of %u (cap %d)", who, result[0], result[1], cap);
  if (fresh) *fresh = (int)result[0];
  if (selected) *selected = m;
  g.fb_pending = false;  // the feedback's pending plane is the filter of the image before the round, whatever the round renders
  if (m == 0) return 0;  // nothing rendered, merged or allocated; E keeps its state
  return history_render_and_merge(g, iter_first, group_iters, m);
}

int pt_ctx_readback_history_extra(PtContext* c, float* extra_host) {
  if (need(c, "pt_readback_history_extra")) return -1;
  Ctx& g = *c;
  if (!extra_host) return pt_fail("pt_readback_history_extra: null buffer");
  if (!g.hist_extra) {
    if (pt_ctx_sync(c)) return -1;
    std::fill(extra_host, extra_host + (size_t)g.N, 0.0f);
    return 0;
  }
  return copy_out(c, "pt_readback_history_extra", extra_host, 1, [&](const float** d) { return *d = g.d_hist_extra, 0; });
}

// ---- the history probes: kept samples rendered again after a move; C.w shortened where they differ ------------------------------
static bool same_camera(const PtCamera& a, const PtCamera& b) {
  return !std::memcmp(a.position, b.position, sizeof a.position) && !std::memcmp(a.view, b.view, sizeof a.view) && !std::memcmp(a.up, b.up, sizeof a.up) &&
         !std::memcmp(a.right, b.right, sizeof a.right) && !std::memcmp(a.fov, b.fov, sizeof a.fov) &&
         !std::memcmp(a.pixelLength, b.pixelLength, sizeof a.pixelLength);
}
static int probe_capacity(const Ctx& g) {  // the probes of phase 0: no phase has more
  const int W = g.cam.resolution[0];
  return pthi::probe_count(pthi::probe_grid(W, g.N / W, 0));
}

int pt_ctx_history_probe_keep(PtContext* c, int iter_first, int iter_count, int phase) {
  const char* who = "pt_history_probe_keep";
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (admit(g, who, kNotFailed)) return -1;
  if (iter_first < 1 || iter_count < 1 || (int64_t)iter_first + iter_count - 1 > INT32_MAX)
    return pt_fail("%s: iterations %d, +%d: the first is >= 1, the count at least one", who, iter_first, iter_count);
  if (phase < 0 || phase > 8) return pt_fail("%s: phase %d is not in 0 .. 8", who, phase);
  if (admit(g, who, kWholeRows) || admit(g, who, kUniform)) return -1;
  if (g.hist_extra)
    return pt_fail("%s: the history round left extra samples in some pixels (pt_history_round): the image is no longer a uniform sum of iterations; call "
                   "pt_history_probe_keep before pt_history_round, or return to the uniform state with pt_clear", who);
  if (!g.d_feat || !g.feat_fresh) return pt_fail(kNoFeatures, who);
  if ((int64_t)iter_count != g.rendered)
    return pt_fail("%s: %d iterations of %d pixels, but %lld iteration(s) have been rendered since the last pt_clear: the probes keep the image's own samples", who,
                   iter_count, g.N, (long long)g.rendered);
  HIP_OK(hipSetDevice(g.device));
  const int W = g.cam.resolution[0], R = g.N / W;
  const int P = pthi::probe_count(pthi::probe_grid(W, R, phase));
  if (ensure(g, g.d_probe, (size_t)probe_capacity(g) * sizeof(pthi::V4), Zero::on_stream)) return -1;  // the first keep of the context
  if (P > 0 && pt_history_probe_keep_launch(g.stream, W, R, phase, g.d_image, reinterpret_cast<const float*>(g.d_feat), g.d_probe)) return -1;
  g.probe_first = iter_first, g.probe_iters = iter_count, g.probe_phase = phase;
  g.probe_N = g.N, g.probe_begin = g.pixel_begin;
  g.probe_cam = g.cam;
  if (g.probe_geoms_stale) g.probe_geoms = g.camera_base.geoms, g.probe_geoms_stale = false;  // retaken only after a pt_set_geoms
  g.probe_geoms_changed = false;
  if (g.probe_materials_stale) g.probe_materials = g.materials, g.probe_materials_stale = false;  // retaken only after a pt_set_materials
  g.probe_materials_changed = false;
  g.probe_kept = true;
  g.probe_checked = false;  // L, if any, was the check of other probes
  return 0;
}

// `moved` of pt_amd.h on the device: all zero unless pt_set_geoms or pt_set_materials has run since the keep; uploaded only when it
// differs from what the device holds (from a member that outlives the copy).
static int probe_moved_table(Ctx& g) {
  const std::vector<PtGeom>& cur = g.camera_base.geoms;
  const size_t n = cur.size();
  std::vector<uint8_t> moved(std::max<size_t>(n, 1), 0);
  if (g.probe_geoms_changed) {
    if (g.probe_geoms.size() == n) pthi::probe_moved(g.probe_geoms.data(), cur.data(), (int)n, moved.data());
    else std::fill(moved.begin(), moved.end(), (uint8_t)1);
  }
  if (g.probe_materials_changed) {  // ... or its material is not what it was at the keep (pthi::recolor_material's mk != 0)
    const std::vector<PtMaterial>&kept = g.probe_materials, &now = g.materials;
    for (size_t i = 0; i < n; ++i) {
      const int32_t m = cur[i].materialid;
      float ratio[3];
      if (kept.size() != now.size()) moved[i] = 1;
      else if (m >= 0 && (size_t)m < now.size() && pthi::recolor_material(kept[(size_t)m], now[(size_t)m], ratio) != pthi::kUnchanged) moved[i] = 1;
    }
  }
  const bool first = !g.d_probe_moved;
  if (ensure(g, g.d_probe_moved, moved.size(), Zero::on_stream)) return -1;
  if (first) g.probe_moved_dev.assign(moved.size(), 0);
  if (moved != g.probe_moved_dev) {
    g.probe_moved_dev = std::move(moved);
    HIP_OK(hipMemcpyAsync(g.d_probe_moved, g.probe_moved_dev.data(), g.probe_moved_dev.size(), hipMemcpyHostToDevice, g.stream));
  }
  return 0;
}

int pt_ctx_history_probe_check(PtContext* c, const PtHistoryProbeOptions* opt, int* probes, int* changed, int* skipped) {
  const char* who = "pt_history_probe_check";
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (admit(g, who, kNotFailed)) return -1;
  if (g.conv) return pt_fail("%s: the renderer was created with PtOptions.convergence = %d; the convergence metric follows whole iterations", who, g.conv);
  if (admit(g, who, kWholeRows) || admit(g, who, kUniform)) return -1;
  if (!g.d_probe || !g.probe_kept) return pt_fail("%s: no probes have been kept (pt_history_probe_keep)", who);
  if (g.probe_N != g.N || g.probe_begin != g.pixel_begin)
    return pt_fail("%s: the probes were kept for a tile of %d pixels from %d, not %d from %d", who, g.probe_N, g.probe_begin, g.N, g.pixel_begin);
  if (!same_camera(g.cam, g.probe_cam))
    return pt_fail("%s: the camera has moved since pt_history_probe_keep: the probes answer for a camera that stands still (keep again after the move)", who);
  if (!g.d_hist || !g.hist_current) return pt_fail("%s: the current plane is absent: no lookup since the last pt_clear or move (pt_history_reproject)", who);
  if (g.probe_applied) return pt_fail("%s: a check has been applied to this current plane already; the next lookup (pt_history_reproject) makes a new one", who);
  if (!g.d_feat || !g.feat_fresh) return pt_fail(kNoFeatures, who);
  pthi::ProbeParams pp{};
  if (pt_history_probe_options(who, opt, &pp)) return -1;
  const int W = g.cam.resolution[0], R = g.N / W;
  const int P = pthi::probe_count(pthi::probe_grid(W, R, g.probe_phase));
  if (probes) *probes = P;
  if (changed) *changed = 0;
  if (skipped) *skipped = 0;
  if (P == 0) return 0;
  HIP_OK(hipSetDevice(g.device));
  const int cap = probe_capacity(g);
  if (ensure(g, g.d_probe_lam, ((size_t)cap + 2) * sizeof(float), Zero::on_stream) || probe_moved_table(g)) return -1;
  if (g.worker && g.worker->capacity >= P) set_worker_live(*g.worker, P);
  else if (ensure_worker(g, P)) return -1;
  const float* feat = reinterpret_cast<const float*>(g.d_feat);
  const int num_geoms = (int)g.camera_base.geoms.size();
  int* counts = reinterpret_cast<int*>(g.d_probe_lam + cap);
  if (pt_history_probe_list_launch(g.stream, W, R, g.probe_phase, g.d_list)) return -1;
  if (render_list(g, g.probe_first, g.probe_iters)) return -1;
  g.samples += (int64_t)g.probe_iters * P;
  if (pt_history_probe_gradient_launch(g.stream, W, R, g.probe_phase, g.d_probe, g.worker->d_image, feat, g.d_probe_moved, num_geoms, g.d_probe_lam, counts))
    return -1;
  if (pt_history_probe_apply_launch(g.stream, W, R, g.probe_phase, g.d_probe_lam, feat, g.d_probe_moved, num_geoms, pp, history_plane(g, pthi::kKeptPlanes)))
    return -1;
  g.probe_checked = g.probe_applied = true;
  int result[2] = {0, 0};  // changed, skipped: 8 bytes and ONE synchronise
  HIP_OK(hipMemcpyAsync(result, counts, sizeof(result), hipMemcpyDeviceToHost, g.stream));
  HIP_OK(hipStreamSynchronize(g.stream));
  if (changed) *changed = result[0];
  if (skipped) *skipped = result[1];
  return 0;
}

int pt_ctx_readback_history_probe(PtContext* c, float* kept, float* lam, int* count) {
  const char* who = "pt_readback_history_probe";
  if (need(c, who)) return -1;
  Ctx& g = *c;
  const int W = g.cam.resolution[0];
  const int P = g.probe_kept ? pthi::probe_count(pthi::probe_grid(W, g.N / W, g.probe_phase)) : 0;
  const bool have_lam = g.probe_checked && g.hist_current && g.d_probe_lam;
  HIP_OK(hipSetDevice(g.device));
  if (kept && P > 0) HIP_OK(hipMemcpyAsync(kept, g.d_probe, (size_t)P * sizeof(pthi::V4), hipMemcpyDeviceToHost, g.stream));
  if (lam && P > 0 && have_lam) HIP_OK(hipMemcpyAsync(lam, g.d_probe_lam, (size_t)P * sizeof(float), hipMemcpyDeviceToHost, g.stream));
  if (pt_ctx_sync(c)) return -1;
  if (lam && !have_lam) std::fill(lam, lam + P, 0.0f);
  if (count) *count = P;
  return 0;
}

// ---- the noise estimate of the blend, and rendering a view until the blend is clean (csrc/pt_noise.hip k_history_noise) ---------
// What both entry points refuse after their own first checks, in the estimate's order: a striped or ragged tile, the adaptive state,
// the extra plane.
static int history_noise_admit(const Ctx& g, const char* who) {
  return admit(g, who, kWholeRows) || admit(g, who, kUniform) || admit(g, who, kNoExtras) ? -1 : 0;
}
static const pthi::V4* history_noise_current(const Ctx& g, int plane) {  // C (0) or VC (1), nullptr while C is absent
  if (!g.hist_current) return nullptr;
  return plane ? history_var_plane(g, 1) : history_plane(g, pthi::kKeptPlanes);
}

int pt_ctx_history_noise(PtContext* c, float samples, uint32_t flags, double* sse) {
  const char* who = "pt_history_noise";
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (admit(g, who, kNotFailed)) return -1;
  if (flags == PT_HISTORY_MOMENTS)
    return pt_fail("%s: PT_HISTORY_MOMENTS is not built: the moments give an estimate only for pixels with four views of history (defined: PT_HISTORY_VARIANCE)", who);
  if (flags != PT_HISTORY_VARIANCE) return pt_fail("%s: flags 0x%x: the only defined value is PT_HISTORY_VARIANCE = 0x%x", who, flags, PT_HISTORY_VARIANCE);
  if (history_noise_admit(g, who)) return -1;
  if (pt_history_check_samples(who, samples)) return -1;
  if (history_folds(g, who, samples) || history_current_variance(g, who)) return -1;
  HIP_OK(hipSetDevice(g.device));
  if (ensure(g, g.d_hist_noise, pt_history_noise_bytes((size_t)g.N))) return -1;  // the first estimate of the context (every word is written before it is read)
  const ptnz::Fold f = ptnz::fold_scalars(1, g.noise_groups, g.noise_iters);
  g.hist_noise = false;
  if (pt_history_noise_launch(g.stream, g.N, g.d_noise, f.Tf, f.Df, samples, history_noise_current(g, 0), history_noise_current(g, 1), g.d_hist_noise)) return -1;
  g.hist_noise = true;
  double result = -1.0;
  HIP_OK(hipMemcpyAsync(&result, pt_history_noise_result(g.d_hist_noise, (size_t)g.N), sizeof(double), hipMemcpyDeviceToHost, g.stream));
  if (pt_ctx_sync(c)) return -1;
  if (sse) *sse = result;
  return 0;
}

int pt_ctx_readback_history_noise(PtContext* c, float* w_host) {
  if (need(c, "pt_readback_history_noise")) return -1;
  return copy_out(c, "pt_readback_history_noise", w_host, 1, [&](const float** d) {
    if (!c->d_hist_noise || !c->hist_noise)
      return pt_fail("pt_readback_history_noise: no estimate has been made since the last pt_clear or move (pt_history_noise)");
    return *d = pt_history_noise_plane(c->d_hist_noise, (size_t)c->N), 0;
  });
}

int pt_ctx_history_render_until(PtContext* c, int iter_first, int max_iters, int group_iters, float target_db, int* iters_done, float* psnr_db,
                                float* view_psnr_db) {
  const char* who = "pt_history_render_until";
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (iter_first < 1 || max_iters < 1 || (int64_t)iter_first + max_iters - 1 > INT32_MAX || group_iters < 0 || !std::isfinite(target_db))
    return pt_fail("%s: iterations %d, +%d in groups of %d until %g dB: the first is >= 1, the count >= 1, the group >= 0 (0 = a batch), the target finite",
                   who, iter_first, max_iters, group_iters, (double)target_db);
  if (admit(g, who, kNotFailed) || history_noise_admit(g, who) || history_current_variance(g, who)) return -1;
  const int group = group_iters ? group_iters : g.K;
  int done = 0;
  float psnr = -1.0f, view_psnr = -1.0f;
  while (done < max_iters) {
    const int n = std::min(group, max_iters - done);
    if (pt_ctx_render(c, iter_first + done, n)) return -1;
    done += n;
    // the fold of pt_ctx_noise_fold and, once it leaves a variance, the estimate of the blend in the same launch
    const int64_t unfolded = g.rendered - g.noise_iters;
    if (unfolded <= 0) continue;
    HIP_OK(hipSetDevice(g.device));
    if (ensure(g, g.d_noise, pt_noise_state_bytes((size_t)g.N), Zero::on_stream)) return -1;
    const ptnz::Fold f = ptnz::fold_scalars(unfolded, g.noise_groups + 1, g.noise_iters + unfolded);
    if (!f.have_variance) {  // one group says nothing about the spread
      if (pt_noise_launch(g.stream, g.N, g.d_image, g.d_noise, f)) return -1;
      g.noise_groups += 1, g.noise_iters += unfolded;
      continue;
    }
    if (ensure(g, g.d_hist_noise, pt_history_noise_bytes((size_t)g.N))) return -1;
    g.hist_noise = false;
    if (pt_noise_fold_history_launch(g.stream, g.N, g.d_image, g.d_noise, f, f.Tf, history_noise_current(g, 0), history_noise_current(g, 1), g.d_hist_noise)) return -1;
    g.noise_groups += 1, g.noise_iters += unfolded;
    g.hist_noise = true;
    double sse[2] = {-1.0, -1.0};  // the view's own, the blend's: 16 bytes and ONE synchronise
    HIP_OK(hipMemcpyAsync(&sse[0], static_cast<const char*>(g.d_noise) + pt_noise_state_bytes((size_t)g.N) - sizeof(double), sizeof(double), hipMemcpyDeviceToHost, g.stream));
    HIP_OK(hipMemcpyAsync(&sse[1], pt_history_noise_result(g.d_hist_noise, (size_t)g.N), sizeof(double), hipMemcpyDeviceToHost, g.stream));
    if (pt_ctx_sync(c)) return -1;
    view_psnr = pt_psnr_from_sse(sse[0], g.N);
    psnr = pt_psnr_from_sse(sse[1], g.N);
    if (psnr > target_db) break;
  }
  if (iters_done) *iters_done = done;
  if (psnr_db) *psnr_db = psnr;
  if (view_psnr_db) *view_psnr_db = view_psnr;
  return 0;
}

// ---- threshold rounds over the blend: the history steps with per-pixel counts (csrc/pt_history_threshold.hip) -----------------------
// What the rounds refuse after the adaptive rounds' own refusals.
static int history_threshold_refusal(const PtContext& g, const char* who) { return history_current_variance(g, who); }
// The counts the steps read: the plane cnt in the adaptive state, else the fold's (T, M) for every pixel.
static const void* history_counts(const Ctx& g) { return g.adaptive ? g.d_acnt : nullptr; }
// What the steps need of the folds in either state: at least two, nothing rendered since, counts that fit an int32.
static int history_counts_folds(const Ctx& g, const char* who) {
  if (!g.d_noise || g.noise_groups < 1) return pt_fail("%s: nothing has been folded (pt_noise_fold)", who);
  if (g.noise_groups < 2) return pt_fail("%s: %d group(s) folded; a variance needs at least 2 (pt_noise_fold after each group of iterations)", who, g.noise_groups);
  if (admit(g, who, kFoldedAll)) return -1;
  if (g.noise_iters > INT32_MAX) return pt_fail("%s: %lld iterations folded: the per-pixel counts are int32", who, (long long)g.noise_iters);
  return 0;
}
// W, the partial sums and NE: from the first call that needs them on (every word is written before it is read)
static int history_noise_ensure(Ctx& g) {
  return ensure(g, g.d_hist_noise, pt_history_noise_bytes((size_t)g.N)) || ensure(g, g.d_hist_ne, (size_t)g.N * sizeof(float)) ? -1 : 0;
}
// Pass A; reduce: with the fold's second launch behind it.
static int history_noise_counts(Ctx& g, bool reduce) {
  g.hist_noise = g.hist_ne = false;
  if (pt_history_noise_counts_launch(g.stream, g.N, g.d_noise, history_counts(g), (int)g.noise_iters, g.noise_groups, history_noise_current(g, 0),
                                     history_noise_current(g, 1), g.d_hist_noise, g.d_hist_ne, reduce))
    return -1;
  g.hist_noise = g.hist_ne = true;
  return 0;
}
// Passes A and B of a round (the context is in the adaptive state, the selection's workspace exists).
static int history_blend_keys(PtContext& g) {
  const int W = g.cam.resolution[0];
  if (history_noise_ensure(g) || history_noise_counts(g, false)) return -1;
  return pt_history_key_blend_launch(g.stream, W, g.N / W, pt_history_noise_plane(g.d_hist_noise, (size_t)g.N), g.d_hist_ne,
                                     pt_adaptive_select_keys(g.d_select, (size_t)g.N));
}
// What the steps refuse in both states, in their order; features: the capture's feature pass.
static int history_counts_refusal(const Ctx& g, const char* who, bool features) {
  if (admit(g, who, kNotFailed) || admit(g, who, kWholeRows)) return -1;
  if (features && (!g.d_feat || !g.feat_fresh)) return pt_fail(kNoFeatures, who);
  if (admit(g, who, kNoExtras) || history_counts_folds(g, who)) return -1;
  return history_current_variance(g, who);
}

int pt_ctx_history_noise_adaptive(PtContext* c, double* sse) {
  const char* who = "pt_history_noise_adaptive";
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (history_counts_refusal(g, who, false)) return -1;
  HIP_OK(hipSetDevice(g.device));
  if (history_noise_ensure(g) || history_noise_counts(g, true)) return -1;
  double result = -1.0;
  HIP_OK(hipMemcpyAsync(&result, pt_history_noise_result(g.d_hist_noise, (size_t)g.N), sizeof(double), hipMemcpyDeviceToHost, g.stream));
  if (pt_ctx_sync(c)) return -1;
  if (sse) *sse = result;
  return 0;
}

int pt_ctx_readback_history_noise_samples(PtContext* c, float* ne_host) {
  if (need(c, "pt_readback_history_noise_samples")) return -1;
  return copy_out(c, "pt_readback_history_noise_samples", ne_host, 1, [&](const float** d) {
    if (!c->d_hist_ne || !c->hist_ne)
      return pt_fail("pt_readback_history_noise_samples: no estimate with per-pixel counts has been made since the last pt_clear, move or round (pt_history_noise_adaptive)");
    return *d = c->d_hist_ne, 0;
  });
}

int pt_ctx_history_resolve_adaptive_device(PtContext* c, const float** rgb_dev) {
  const char* who = "pt_history_resolve_adaptive";
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (history_counts_refusal(g, who, false)) return -1;
  if (!rgb_dev) return pt_fail("%s: null buffer", who);
  HIP_OK(hipSetDevice(g.device));
  if (ensure(g, g.d_resolved, 3 * (size_t)g.N * sizeof(float))) return -1;
  if (pt_history_blend_counts_launch(g.stream, g.N, g.d_image, history_counts(g), (int)g.noise_iters, g.noise_groups, history_noise_current(g, 0), g.d_resolved))
    return -1;
  *rgb_dev = g.d_resolved;
  return 0;
}
int pt_ctx_history_resolve_adaptive(PtContext* c, float* rgb_avg_host) {
  const char* who = "pt_history_resolve_adaptive";
  if (need(c, who)) return -1;
  if (history_counts_refusal(*c, who, false)) return -1;  // (before the null buffer)
  return copy_out(c, who, rgb_avg_host, 3, [&](const float** d) { return pt_ctx_history_resolve_adaptive_device(c, d); });
}

int pt_ctx_history_capture_adaptive(PtContext* c) {
  const char* who = "pt_history_capture_adaptive";
  if (need(c, who)) return -1;
  Ctx& g = *c;
  if (history_counts_refusal(g, who, true)) return -1;
  HIP_OK(hipSetDevice(g.device));
  if (ensure(g, g.d_hist, pt_history_state_bytes((size_t)g.N), Zero::on_stream)) return -1;  // the first capture of the context
  if (ensure(g, g.d_hist_var, pt_history_variance_bytes((size_t)g.N), Zero::on_stream)) return -1;
  if (pt_history_capture_counts_launch(g.stream, g.N, g.d_image, reinterpret_cast<const float*>(g.d_feat), g.d_noise, history_counts(g), (int)g.noise_iters,
                                       g.noise_groups, history_noise_current(g, 0), history_noise_current(g, 1), g.d_hist, history_var_plane(g, 0)))
    return -1;
  g.hist_cam = g.cam;
  if (PtHistoryMotion& hm = g.hist_motion; hm.geoms_stale) hm.geoms = g.camera_base.geoms, hm.geoms_stale = false, hm.fresh = false;  // as in any capture
  if (PtHistoryMaterials& hm = g.hist_materials; hm.stale) hm.materials = g.materials, hm.stale = false, hm.fresh = false;  // ... and the materials
  g.hist_kept = true;
  g.hist_var_kept = PT_HISTORY_VARIANCE;
  g.fb_kept = false;  // kept without feedback
  return 0;
}

// The guided filter over the blend with per-pixel counts (ptdn::Form::HistoryAdaptive): everything it refuses but the null buffer, in
// pt_history_denoise's order without the adaptive state and `samples`; the job resolved.
static int history_denoise_adaptive_refusal(const Ctx& g, const char* who, const PtDenoiseOptions* opt, ptdn::Job* j) {
  if (admit(g, who, kNotFailed) || admit(g, who, kWholeRows) || admit(g, who, kNoExtras)) return -1;
  if (!g.d_feat || !g.feat_fresh) return pt_fail(kNoFeatures, who);
  ptdn::Params P{};
  if (const char* msg = ptdn::resolve(opt, &P, ptdn::kHistorySigmaColor)) return pt_fail("%s: %s", who, msg);
  if (history_counts_folds(g, who) || history_current_variance(g, who)) return -1;
  return pt_denoise_resolve(who, ptdn::Form::HistoryAdaptive, 0.0f, g.noise_groups, g.noise_iters, opt, j);
}
int pt_ctx_history_denoise_adaptive_device(PtContext* c, const PtDenoiseOptions* opt, const float** rgb_dev) {
  const char* who = "pt_history_denoise_adaptive";
  if (need(c, who)) return -1;
  Ctx& g = *c;
  ptdn::Job j{};
  if (history_denoise_adaptive_refusal(g, who, opt, &j)) return -1;
  if (!rgb_dev) return pt_fail("%s: null buffer", who);
  HIP_OK(hipSetDevice(g.device));
  if (ensure(g, g.d_denoise, pt_denoise_workspace_bytes((size_t)g.N))) return -1;  // the first denoise call of the context, of any kind
  const int W = g.cam.resolution[0];
  j.f = {W, g.N / W, g.d_image, reinterpret_cast<const float*>(g.d_feat), static_cast<const float*>(g.d_noise)};
  j.div.cnt = static_cast<const ptad::Cnt*>(history_counts(g));
  if (g.hist_current) {
    j.div.C = reinterpret_cast<const ptdn::V4*>(history_plane(g, pthi::kKeptPlanes));
    j.div.VC = reinterpret_cast<const ptdn::V4*>(history_var_plane(g, 1));
  }
  return pt_denoise_launch(g.stream, j, g.d_denoise, rgb_dev);
}
int pt_ctx_history_denoise_adaptive(PtContext* c, const PtDenoiseOptions* opt, float* rgb_avg_host) {
  const char* who = "pt_history_denoise_adaptive";
  if (need(c, who)) return -1;
  ptdn::Job j{};
  if (history_denoise_adaptive_refusal(*c, who, opt, &j)) return -1;  // (before the null buffer)
  return copy_out(c, who, rgb_avg_host, 3, [&](const float** d) { return pt_ctx_history_denoise_adaptive_device(c, opt, d); });
}

int pt_ctx_history_drop(PtContext* c) {
  if (need(c, "pt_history_drop")) return -1;
  Ctx& g = *c;
  if (g.d_hist) {  // forgotten, not freed: a readback sees zeros, a reprojection has nothing to read
    HIP_OK(hipSetDevice(g.device));
    HIP_OK(hipMemsetAsync(g.d_hist, 0, pt_history_state_bytes((size_t)g.N), g.stream));
    if (g.d_hist_var) HIP_OK(hipMemsetAsync(g.d_hist_var, 0, pt_history_variance_bytes((size_t)g.N), g.stream));
  }
  g.hist_kept = g.hist_current = false;
  g.hist_var_kept = g.hist_var_current = 0;
  g.fb_kept = g.fb_current = g.fb_pending = false;  // the feedback's three planes are forgotten with K
  g.probe_kept = g.probe_checked = g.probe_applied = false;  // the probes are forgotten with K, their L with C
  return 0;
}

}  // extern "C"
