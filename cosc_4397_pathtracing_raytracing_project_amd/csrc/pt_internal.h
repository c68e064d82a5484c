// pt_internal.h — shared by the translation units of libpt_amd.so (not part of the ABI).
#pragma once
int pt_fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));  // sets pt_last_error(), returns -1

// The edge-avoiding filter in its three forms (pt_denoise.hip; ptdn::Form and ptdn::Job: pt_denoise.h), on raw device pointers and a stream
// so that a context (its tile) and a group (the frame assembled on the root device) run the same launches.
// pt_denoise_resolve: the options and the form's counters (plain: samples; guided: the fold counters M = groups, T = iters; adaptive: the
// same two for every pixel of the uniform state) -> j->form, j->P and j->div, the rest of *j zero, or the refusal.
// pt_denoise_adaptive_check: what the host and stage entries of the adaptive form refuse in their arrays (counts: w*rows * {T_p, M_p},
// the first pixel with M_p < 2 or T_p < M_p is named), then the options.
// pt_denoise_launch: j.w x j.rows pixels; j.rgb_sum w*rows*3 floats, j.planes PT_FEATURE_PLANES * w*rows float4, j.noise (the guided
// forms) the fold's PT_NOISE_PLANES planes, j.div.cnt (the adaptive form) the plane `cnt` of adaptive sampling or nullptr: every pixel
// has (div.T, div.M); workspace_dev pt_denoise_workspace_bytes(w * rows) bytes; asynchronous on `stream`; *rgb_avg_dev (w*rows*3 floats)
// points into the workspace.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
struct PtDenoiseOptions;
namespace ptdn {
enum class Form;
struct Job;
}
inline size_t pt_denoise_workspace_bytes(size_t pixels) { return 80 * pixels; }
int pt_denoise_resolve(const char* who, ptdn::Form form, float samples, int groups, int64_t iters, const PtDenoiseOptions* opt, ptdn::Job* j);
int pt_denoise_adaptive_check(const char* who, int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                              const PtDenoiseOptions* opt, ptdn::Job* j);
int pt_denoise_launch(hipStream_t stream, const ptdn::Job& j, void* workspace_dev, const float** rgb_avg_dev);
// The history form (ptdn::Form::History, pt_history_denoise): what its host and stage entries refuse, in pt_history_denoise's order, and
// the job resolved; a launch reads the planes C and VC from j->div.C and j->div.VC (both or neither), the host loop from j->f.
int pt_history_denoise_check(const char* who, int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups, int64_t iters,
                             float samples, const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, const float* rgb_avg, ptdn::Job* j);
// The history form with per-pixel counts (ptdn::Form::HistoryAdaptive, pt_history_denoise_adaptive): the same for it; counts as
// pt_denoise_adaptive_check reads them, and a launch reads the count plane from j->div.cnt (nullptr: (div.T, div.M) for every pixel).
int pt_history_denoise_adaptive_check(const char* who, int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                                      const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, bool has_output, ptdn::Job* j);
// The moments form (ptdn::Form::Moments, pt_history_denoise_ex with PT_HISTORY_MOMENTS): the same for it; no fold, no noise planes.
// has_output: the caller gave a buffer to write to.
int pt_history_denoise_moments_check(const char* who, int w, int rows, const float* rgb_sum, const float* planes, float samples, const float* current_plane,
                                     const float* current_var, const PtDenoiseOptions* opt, bool has_output, ptdn::Job* j);

// The feedback form (ptdn::Form::Feedback, pt_history_denoise_feedback): the moments form's refusals, then fb out of range (level 1 ..
// the filter's levels, variance 1 or -1 for rule 0; 0 / NULL: the defaults) and C without FC; j->tap_level and j->div.fb_variance (the
// rule, 0 or 1) resolved.
// A launch reads FC from j->div.FC and writes the pending plane j->tap (w * rows float4) after level j->tap_level - 1.
struct PtHistoryFeedbackOptions;
int pt_history_feedback_options(const char* who, const PtHistoryFeedbackOptions* fb, int levels, int* level, int* variance);
int pt_history_denoise_feedback_check(const char* who, int w, int rows, const float* rgb_sum, const float* planes, float samples, const float* current_plane,
                                      const float* current_var, const float* current_fb, const PtDenoiseOptions* opt, const PtHistoryFeedbackOptions* fb,
                                      bool has_output, ptdn::Job* j);

// The noise estimate (pt_noise.hip), on raw device pointers and a stream.  state_dev holds pt_noise_state_bytes(pixels) bytes:
// PT_NOISE_PLANES planes of `pixels` float4, then one double per PT_NOISE_PIXELS_PER_PARTIAL pixels (k_noise_fold's partial sums),
// then the double they add up to (k_noise_reduce).  pt_noise_launch: one fold of the SUM image rgb_sum_dev (pixels * 3 floats) with the
// scalars of ptnz::fold_scalars; asynchronous on `stream`.
namespace ptnz {
struct Fold;
}
inline size_t pt_noise_partials(size_t pixels) { return (pixels + 1023) / 1024; }
inline size_t pt_noise_state_bytes(size_t pixels) { return 32 * pixels + 8 * (pt_noise_partials(pixels) + 1); }
struct PtContext;
int64_t pt_ctx_unfolded_iterations(const PtContext* c);  // iterations rendered since the context's last fold
int pt_noise_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, void* state_dev, const ptnz::Fold& f);
// k_noise_reduce alone: *sse_dev = partial_dev[0] + ... + partial_dev[count - 1] in index order (one thread adds).
int pt_noise_reduce_launch(hipStream_t stream, int count, const double* partial_dev, double* sse_dev);
// The noise estimate of the blend (pt_history_noise; pt_noise.hip k_history_noise).  out_dev holds pt_history_noise_bytes(pixels)
// bytes: one double per PT_NOISE_PIXELS_PER_PARTIAL pixels, the double they add up to (pt_history_noise_result), then the plane W of
// `pixels` floats (the doubles first: 4 * pixels is no multiple of 8 for an odd tile).  state_dev: the fold's state; Tf, Df:
// ptnz::fold_scalars' of the folds so far; current_dev / current_var_dev: C and VC, both or neither.
// pt_noise_fold_history_launch: pt_noise_launch and pt_history_noise_launch as ONE kernel and the two reductions; f.have_variance.
inline size_t pt_history_noise_bytes(size_t pixels) { return 4 * pixels + 8 * (pt_noise_partials(pixels) + 1); }
inline const double* pt_history_noise_result(const void* out_dev, size_t pixels) { return static_cast<const double*>(out_dev) + pt_noise_partials(pixels); }
inline float* pt_history_noise_plane(void* out_dev, size_t pixels) { return reinterpret_cast<float*>(static_cast<double*>(out_dev) + pt_noise_partials(pixels) + 1); }
int pt_history_noise_launch(hipStream_t stream, int pixels, const void* state_dev, float Tf, float Df, float samples, const void* current_dev,
                            const void* current_var_dev, void* out_dev);
int pt_noise_fold_history_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, void* state_dev, const ptnz::Fold& f, float samples,
                                 const void* current_dev, const void* current_var_dev, void* out_dev);
int pt_history_noise_check(const char* who, int pixels, const float* noise_planes, int groups, int64_t iters, float samples, const float* current_plane,
                           const float* current_var);

// Adaptive sampling (pt_adaptive.hip), on raw device pointers and a stream; everything asynchronous, nothing allocated.
// counts_dev: the plane `cnt`, pixels * {int32 T_p, int32 M_p}.  noise_dev / noise_state_dev: the fold's state (pt_noise_state_bytes).
// pt_adaptive_select_launch: the m pixels of a tile of w x rows with the largest key -> list_dev (m entries, ascending tile index);
// workspace_dev holds pt_adaptive_select_bytes(pixels) bytes.  pt_adaptive_merge_launch: group_sum_dev (m * 3 floats, the worker's
// sums of group_iters iterations for the pixels of list_dev) joins the image, the planes and the counts; leaves SSE_est where a
// fold leaves it.  pt_adaptive_resolve_launch: rgb_avg_dev = S / (float)T_p (counts_dev == nullptr: T_p = iters for every pixel).
size_t pt_adaptive_select_bytes(size_t pixels);
int pt_adaptive_check_select(const char* who, int w, int rows, const float* noise_planes, const int32_t* counts, int m, const int32_t* list);
int pt_adaptive_init_counts_launch(hipStream_t stream, int pixels, void* counts_dev, int iters, int groups);
int pt_adaptive_select_launch(hipStream_t stream, int w, int rows, const float* noise_dev, const void* counts_dev, int m, void* workspace_dev,
                              int32_t* list_dev);
// Selection by threshold: the pixels whose key exceeds threshold * threshold, the `cap` with the largest keys at the most, at the
// front of list_dev (cap entries; those behind the list's length keep what they held).  pt_adaptive_select_result: two uint32 in the
// workspace, {above, m = min(above, cap)}, valid once the launches have run.
int pt_adaptive_check_threshold(const char* who, float threshold);  // finite and >= 0, or the refusal
int pt_adaptive_select_threshold_launch(hipStream_t stream, int w, int rows, const float* noise_dev, const void* counts_dev, float threshold, int cap,
                                        void* workspace_dev, int32_t* list_dev);
const uint32_t* pt_adaptive_select_result(const void* workspace_dev, size_t pixels);
// The same selection from keys that are in the workspace already: pt_adaptive_select_keys names the w*rows words a caller fills on
// `stream` before the launches (pt_group_select.hip: the keys of a frame whose noise planes lie on several devices).
uint32_t* pt_adaptive_select_keys(void* workspace_dev, size_t pixels);
int pt_adaptive_select_threshold_keys_launch(hipStream_t stream, int w, int rows, float threshold, int cap, void* workspace_dev, int32_t* list_dev);
int pt_adaptive_merge_launch(hipStream_t stream, int pixels, float* rgb_sum_dev, void* noise_state_dev, void* counts_dev, const int32_t* list_dev, int m,
                             const float* group_sum_dev, int group_iters);
int pt_adaptive_resolve_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const void* counts_dev, int iters, float* rgb_avg_dev);

// Adaptive sampling across a group of contexts (pt_group_select.hip), on raw device pointers and a stream; asynchronous, nothing allocated.
// pt_group_pack_launch: packed_dev[p] = {w_p, T_p} of a tile (8 bytes per pixel) from plane 0 of noise_dev and counts_dev.
// pt_group_keys_launch: the selection keys of a frame of w x rows pixels from its packed pairs -> key_dev (pt_adaptive_select_keys).
// pt_group_partition_launch: the first m = select_result_dev[1] entries of list_dev (ascending frame pixels of a frame w wide, at most
// max_entries of them; select_result_dev = pt_adaptive_select_result's {above, m}) cut for n contexts -> parts_dev, the parts back to back;
// result_dev receives 2 + n words {above, m, m_0 .. m_(n-1)}; workspace_dev holds pt_group_partition_bytes(max_entries, n) bytes.
// pt_group_offsets_launch: offsets_dev[i] = the frame offset of tile pixel list_dev[i] on a striped tile (ptgs::stripe_offset), i < m.
int pt_group_pack_launch(hipStream_t stream, int pixels, const float* noise_dev, const void* counts_dev, void* packed_dev);
int pt_group_keys_launch(hipStream_t stream, int w, int rows, const void* packed_dev, uint32_t* key_dev);
size_t pt_group_partition_bytes(size_t max_entries, int n);
int pt_group_partition_launch(hipStream_t stream, int w, int n, const int32_t* list_dev, const uint32_t* select_result_dev, int max_entries,
                              void* workspace_dev, int32_t* parts_dev, uint32_t* result_dev);
int pt_group_offsets_launch(hipStream_t stream, const int32_t* list_dev, int m, int stripe, int gap, int32_t* offsets_dev);
// what the host and stage forms of the partition refuse
int pt_group_partition_check(const char* who, int w, int h, int n, const int32_t* list, int m, const int32_t* parts, const int32_t* counts);

// The reprojected sample history (pt_history.hip), on raw device pointers and a stream; everything asynchronous, nothing allocated.
// state: pt_history_state_bytes(pixels) bytes, the kept planes K0 K1 K2 and the current plane C, `pixels` float4 each.  current_dev may
// be nullptr in the capture and the blend: C absent, all zero.  pt_history_reproject_launch: v = pthi::make_view(kept camera, rows, row0);
// reject_dev one byte per geom.  pt_history_check_samples / _resolve_options / _reproject_check: the refusals under the name `who`.
struct PtCamera;
struct PtHistoryOptions;
namespace pthi {
struct Params;
struct View;
}
inline size_t pt_history_state_bytes(size_t pixels) { return 64 * pixels; }
inline size_t pt_history_variance_bytes(size_t pixels) { return 32 * pixels; }  // the variance state: VK, then VC, `pixels` float4 each
int pt_history_check_samples(const char* who, float samples);
int pt_history_check_fold_samples(const char* who, float samples, int64_t iters);  // samples == (float)iters, or the refusal
int pt_history_resolve_options(const char* who, const PtHistoryOptions* opt, pthi::Params* P);
int pt_history_reproject_check(const char* who, int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                               const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* current_plane, pthi::Params* P);
int pt_history_capture_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const float* planes_dev, const void* current_dev, float samples,
                              void* kept_dev);
int pt_history_reproject_launch(hipStream_t stream, const pthi::View& v, const void* kept_dev, const float* planes_dev, const uint8_t* reject_dev,
                                int num_geoms, const pthi::Params& P, void* current_dev);
// The same two with the variance side (PT_HISTORY_VARIANCE): the fold's planes and ptnz::fold_scalars' Tf, Df; VC beside C (both or
// neither) and VK in the capture, VK and VC in the reprojection.  C and K are what the plain launches write, bit for bit.
int pt_history_capture_variance_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const float* planes_dev, const void* current_dev, float samples,
                                       void* kept_dev, const float* noise_dev, float Tf, float Df, const void* current_var_dev, void* kept_var_dev);
int pt_history_reproject_variance_launch(hipStream_t stream, const pthi::View& v, const void* kept_dev, const float* planes_dev, const uint8_t* reject_dev,
                                         int num_geoms, const pthi::Params& P, void* current_dev, const void* kept_var_dev, void* current_var_dev);
// The capture with the moments side (PT_HISTORY_MOMENTS): VC beside C (both or neither) and VK = {m2b.xyz, rb}; no fold is read.  The
// lookup with moments interpolates all four components of VK (a kernel instantiation of its own; the variance kind's is untouched).
int pt_history_capture_moments_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const float* planes_dev, const void* current_dev, float samples,
                                      void* kept_dev, const void* current_var_dev, void* kept_var_dev);
int pt_history_reproject_moments_launch(hipStream_t stream, const pthi::View& v, const void* kept_dev, const float* planes_dev, const uint8_t* reject_dev,
                                        int num_geoms, const pthi::Params& P, void* current_dev, const void* kept_var_dev, void* current_var_dev);
// The lookup with the objects' motion (PT_HISTORY_MOTION): kind 0 (plain), PT_HISTORY_VARIANCE or PT_HISTORY_MOMENTS; table_dev
// pthi::kMotionRow floats and kind_dev one byte per geom (num_geoms >= 1); kept_var_dev / current_var_dev nullptr for kind 0.
int pt_history_reproject_motion_launch(hipStream_t stream, uint32_t kind, const pthi::View& v, const void* kept_dev, const float* planes_dev,
                                       const uint8_t* reject_dev, int num_geoms, const pthi::Params& P, void* current_dev, const void* kept_var_dev,
                                       void* current_var_dev, const float* table_dev, const uint8_t* kind_dev);
// What the host and stage forms of that lookup refuse after pt_history_reproject_check: the flag word, the table, the kinds, VK / VC.
int pt_history_motion_check(const char* who, uint32_t flags, int num_geoms, const float* table, const uint8_t* kind, const float* kept_var,
                            const float* current_var);
// The lookup with the materials' edits (PT_HISTORY_MATERIALS): kind as above; recolor_dev pthi::kRecolorRow floats (16-byte aligned) and
// rkind_dev one byte per geom (num_geoms >= 1); table_dev and kind_dev as above, or both nullptr (nothing moved, or no PT_HISTORY_MOTION).
int pt_history_reproject_materials_launch(hipStream_t stream, uint32_t kind, const pthi::View& v, const void* kept_dev, const float* planes_dev,
                                          const uint8_t* reject_dev, int num_geoms, const pthi::Params& P, void* current_dev, const void* kept_var_dev,
                                          void* current_var_dev, const float* table_dev, const uint8_t* kind_dev, const float* recolor_dev, const uint8_t* rkind_dev);
// What the host and stage forms of that lookup refuse after pt_history_reproject_check: the flag word, the tables, the kinds, VK / VC.
int pt_history_materials_check(const char* who, uint32_t flags, int num_geoms, const float* table, const uint8_t* kind, const float* recolor, const uint8_t* rkind,
                               const float* kept_var, const float* current_var);
// The moments lookup with the filtered colour (PT_HISTORY_FEEDBACK): FK beside VK, FC beside VC, `pixels` float4 each; table_dev and
// kind_dev as above, or both nullptr (nothing moved).  C and VC are the bits pt_history_reproject_moments_launch / _motion_launch write.
inline size_t pt_history_feedback_bytes(size_t pixels) { return 48 * pixels; }  // the feedback state: three planes, the roles FK, FC and P
int pt_history_reproject_feedback_launch(hipStream_t stream, const pthi::View& v, const void* kept_dev, const float* planes_dev, const uint8_t* reject_dev,
                                         int num_geoms, const pthi::Params& P, void* current_dev, const void* kept_var_dev, void* current_var_dev,
                                         const void* kept_fb_dev, void* current_fb_dev, const float* table_dev, const uint8_t* kind_dev);
int pt_history_reproject_feedback_check(const char* who, int num_geoms, const float* kept_var, const float* kept_fb, const float* table, const uint8_t* kind,
                                        const float* current_var, const float* current_fb);
int pt_history_blend_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, float samples, const void* current_dev, float* rgb_avg_dev);
// The history round (pt_history_round): the key of every tile pixel into key_dev (pt_adaptive_select_keys of the selection's workspace;
// emitter_dev one byte per geom), the merge of the worker's group sum (m >= 1 list entries) into the image and the extra plane E
// (`pixels` floats), and the counted forms of capture and blend, which read ns = samples + E_p for `samples`.  The checks: what the
// host and stage forms refuse, under the name `who`.
struct PtHistoryRoundOptions;
namespace pthi {
struct RoundParams;
}
int pt_history_round_options(const char* who, const PtHistoryRoundOptions* opt, pthi::RoundParams* P);
// The history probes (pt_history_probe_keep / _check) of a tile of w x rows at `phase` with at least one probe: probe_dev PK (16 B per
// probe), list_dev the rounds' list, group_sum_dev the worker's sum, lam_dev L, counts_dev two int32 (zeroed by the gradient's launch),
// moved_dev one byte per geom.
struct PtHistoryProbeOptions;
namespace pthi {
struct ProbeParams;
}
int pt_history_probe_options(const char* who, const PtHistoryProbeOptions* opt, pthi::ProbeParams* P);
int pt_history_probe_keep_launch(hipStream_t stream, int w, int rows, int phase, const float* rgb_sum_dev, const float* planes_dev, void* probe_dev);
int pt_history_probe_list_launch(hipStream_t stream, int w, int rows, int phase, int32_t* list_dev);
int pt_history_probe_gradient_launch(hipStream_t stream, int w, int rows, int phase, const void* probe_dev, const float* group_sum_dev, const float* planes_dev,
                                     const uint8_t* moved_dev, int num_geoms, float* lam_dev, int* counts_dev);
int pt_history_probe_apply_launch(hipStream_t stream, int w, int rows, int phase, const float* lam_dev, const float* planes_dev, const uint8_t* moved_dev,
                                  int num_geoms, const pthi::ProbeParams& P, void* current_dev);
int pt_history_select_check(const char* who, int w, int rows, const float* feature_planes, const uint8_t* emitter_geom, int num_geoms,
                            const PtHistoryRoundOptions* opt, const int32_t* list, const int* fresh, const int* m, pthi::RoundParams* P, int* cap);
int pt_history_merge_check(const char* who, int pixels, const float* rgb_sum, const float* extra, const int32_t* list, int m, const float* group_sum,
                           int group_iters);
int pt_history_check_extra(const char* who, int pixels, const float* extra);
int pt_history_key_launch(hipStream_t stream, int pixels, const float* planes_dev, const void* current_dev, const uint8_t* emitter_dev, int num_geoms,
                          float min_history, uint32_t* key_dev);
int pt_history_merge_launch(hipStream_t stream, int pixels, float* rgb_sum_dev, float* extra_dev, const int32_t* list_dev, int m, const float* group_sum_dev,
                            int group_iters);
int pt_history_capture_counted_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const float* planes_dev, const void* current_dev, float samples,
                                      const float* extra_dev, void* kept_dev);
int pt_history_capture_moments_counted_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const float* planes_dev, const void* current_dev,
                                              float samples, const float* extra_dev, void* kept_dev, const void* current_var_dev, void* kept_var_dev);
int pt_history_blend_counted_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, float samples, const float* extra_dev, const void* current_dev,
                                    float* rgb_avg_dev);

// Threshold rounds over the blend (pt_history_round_threshold; pt_history_threshold.hip): the history steps with per-pixel counts.
// counts_dev: the plane `cnt` of the adaptive state, or nullptr: every pixel has the fold's (iters, groups), groups >= 2.
// pt_history_noise_counts_launch: pass A — W into out_dev's plane (pt_history_noise_plane) and the partial sums in front of it, NE into
// ne_dev (`pixels` floats); reduce: k_noise_reduce leaves their sum at pt_history_noise_result.  pt_history_key_blend_launch: pass B,
// the keys of a tile of w x rows from W and NE into key_dev (pt_adaptive_select_keys).  The blend and the capture read Tf_p from the counts;
// the capture writes K (three planes) and VK.  pt_history_counts_check: what the host and stage forms refuse in their counts.
int pt_history_noise_counts_launch(hipStream_t stream, int pixels, const void* state_dev, const void* counts_dev, int iters, int groups, const void* current_dev,
                                   const void* current_var_dev, void* out_dev, float* ne_dev, bool reduce);
int pt_history_key_blend_launch(hipStream_t stream, int w, int rows, const float* w_dev, const float* ne_dev, uint32_t* key_dev);
int pt_history_blend_counts_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const void* counts_dev, int iters, int groups,
                                   const void* current_dev, float* rgb_avg_dev);
int pt_history_capture_counts_launch(hipStream_t stream, int pixels, const float* rgb_sum_dev, const float* planes_dev, const void* state_dev,
                                     const void* counts_dev, int iters, int groups, const void* current_dev, const void* current_var_dev, void* kept_dev,
                                     void* kept_var_dev);
int pt_history_counts_check(const char* who, int pixels, const int32_t* counts, const float* current_plane, const float* current_var);
