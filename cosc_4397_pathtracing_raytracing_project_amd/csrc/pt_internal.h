// pt_internal.h — shared by the translation units of libpt_amd.so (not part of the ABI).
#pragma once
int pt_fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));  // sets pt_last_error(), returns -1

// The edge-avoiding filter (pt_denoise.hip), on raw device pointers and a stream so that a context (its tile) and a group (the frame
// assembled on the root device) run the same launches.  pt_denoise_resolve: samples and options -> parameters, or the refusal.
// pt_denoise_launch: w x rows pixels; rgb_sum_dev w*rows*3 floats, planes_dev PT_FEATURE_PLANES * w*rows float4, workspace_dev
// pt_denoise_workspace_bytes(w * rows) bytes; asynchronous on `stream`; *rgb_avg_dev (w*rows*3 floats) points into the workspace.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
struct PtDenoiseOptions;
namespace ptdn {
struct Params;
}
inline size_t pt_denoise_workspace_bytes(size_t pixels) { return 80 * pixels; }
int pt_denoise_resolve(const char* who, float samples, const PtDenoiseOptions* opt, ptdn::Params* P);
int pt_denoise_launch(hipStream_t stream, int w, int rows, const float* rgb_sum_dev, const float* planes_dev, float samples, const ptdn::Params& P,
                      void* workspace_dev, const float** rgb_avg_dev);
// The variance-guided form (pt_denoise_guided).  pt_denoise_guided_resolve: the fold counters M, T and the options -> parameters and
// ptnz::fold_scalars' Tf, Df, or the refusal.  pt_denoise_guided_launch: as pt_denoise_launch, plus noise_dev, the fold's
// PT_NOISE_PLANES planes of w*rows float4; same workspace.
int pt_denoise_guided_resolve(const char* who, int groups, int64_t iters, const PtDenoiseOptions* opt, ptdn::Params* P, float* Tf, float* Df);
int pt_denoise_guided_launch(hipStream_t stream, int w, int rows, const float* rgb_sum_dev, const float* planes_dev, const float* noise_dev, float Tf,
                             float Df, const ptdn::Params& P, void* workspace_dev, const float** rgb_avg_dev);

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
