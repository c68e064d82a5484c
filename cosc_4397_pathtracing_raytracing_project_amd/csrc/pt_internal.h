// pt_internal.h — shared by the translation units of libpt_amd.so (not part of the ABI).
#pragma once
int pt_fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));  // sets pt_last_error(), returns -1

// The edge-avoiding filter (pt_denoise.hip), on raw device pointers and a stream so that a context (its tile) and a group (the frame
// assembled on the root device) run the same launches.  pt_denoise_resolve: samples and options -> parameters, or the refusal.
// pt_denoise_launch: w x rows pixels; rgb_sum_dev w*rows*3 floats, planes_dev PT_FEATURE_PLANES * w*rows float4, workspace_dev
// pt_denoise_workspace_bytes(w * rows) bytes; asynchronous on `stream`; *rgb_avg_dev (w*rows*3 floats) points into the workspace.
#include <hip/hip_runtime.h>

#include <cstddef>
struct PtDenoiseOptions;
namespace ptdn {
struct Params;
}
inline size_t pt_denoise_workspace_bytes(size_t pixels) { return 80 * pixels; }
int pt_denoise_resolve(const char* who, float samples, const PtDenoiseOptions* opt, ptdn::Params* P);
int pt_denoise_launch(hipStream_t stream, int w, int rows, const float* rgb_sum_dev, const float* planes_dev, float samples, const ptdn::Params& P,
                      void* workspace_dev, const float** rgb_avg_dev);
