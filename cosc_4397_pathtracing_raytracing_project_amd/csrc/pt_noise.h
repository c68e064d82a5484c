// pt_noise.h — the noise estimate of include/pt_amd.h (pt_noise_fold), ONE implementation of its arithmetic.
//
// fold_pixel below is what the HIP kernel (pt_noise.hip k_noise_fold) and the host loop (fold_host, exported as pt_noise_fold_host)
// both run, so the two cannot disagree; tests/noise_ref.py restates it in numpy.  Every float operation is a separate IEEE operation
// in the order pt_amd.h states (`#pragma clang fp contract(off)`, correctly rounded division, denormals kept), so the planes do not
// depend on the arithmetic mode of the build or on the side the fold runs on.  Plain C++ apart from PT_HD.
//
// The estimator: the SUM image S is looked at only at group boundaries.  With B_j = S_j - S_(j-1) the sum of the n_j samples of
// group j, q = sum_j B_j^2 / n_j and T = sum_j n_j,  E[q - S^2 / T] = (M - 1) sigma^2  for any group sizes, so
// v = max(q - S^2 / T, 0) / ((M - 1) T) estimates sigma^2 / T, the variance of the pixel's average.  Per pixel the state is the
// previous S and q: 32 bytes in two float4 planes, whose spare words carry the estimate w = v_x + v_y + v_z and a zero.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/pt_amd.h"
#include "pt_portable_math.h"

namespace ptnz {

struct alignas(16) V4 {  // the device's planes: one 16-byte load or store per pixel and plane
  float x, y, z, w;
};
struct F4 {  // a caller's host array of floats promises no more than float alignment
  float x, y, z, w;
};
static_assert(PT_NOISE_PLANES * sizeof(V4) == 32, "pt_amd.h documents 32 bytes of state per pixel");

// The scalars of one fold: the group's n, and T and M AFTER it (pt_amd.h).  Df is a float32 product.
struct Fold {
  float nf, Tf, Df;
  int have_variance;  // M >= 2
};
inline Fold fold_scalars(int64_t group_iters, int groups_after, int64_t iters_after) {
#pragma clang fp contract(off)
  const float Tf = (float)iters_after;
  return Fold{(float)group_iters, Tf, (float)(groups_after - 1) * Tf, groups_after >= 2 ? 1 : 0};
}

// One colour component: the new q, and (M >= 2) the variance estimate of the average
PT_HD float fold_component(float s, float prev, float* q, const Fold& f) {
#pragma clang fp contract(off)
  const float b = s - prev;
  *q = *q + (b * b) / f.nf;
  if (!f.have_variance) return 0.0f;
  const float d = *q - (s * s) / f.Tf;
  return (d > 0.0f ? d : 0.0f) / f.Df;
}

// Pixel i of a tile of npix pixels: S holds npix * 3 floats, planes PT_NOISE_PLANES * npix float4 (P4: V4 or F4).  Returns w.
// kept (or nullptr): receives the two words the pixel's planes now hold, for a caller that goes on with them (k_noise_fold_history).
template <typename P4>
PT_HD float fold_pixel(size_t i, size_t npix, const float* S, P4* planes, const Fold& f, P4* kept = nullptr) {
#pragma clang fp contract(off)
  const float sx = S[3 * i], sy = S[3 * i + 1], sz = S[3 * i + 2];
  const P4 prev = planes[i];
  P4 q = planes[npix + i];
  const float vx = fold_component(sx, prev.x, &q.x, f);
  const float vy = fold_component(sy, prev.y, &q.y, f);
  const float vz = fold_component(sz, prev.z, &q.z, f);
  const float w = f.have_variance ? (vx + vy) + vz : 0.0f;
  planes[i] = P4{sx, sy, sz, w};
  planes[npix + i] = P4{q.x, q.y, q.z, 0.0f};
  if (kept) kept[0] = P4{sx, sy, sz, w}, kept[1] = P4{q.x, q.y, q.z, 0.0f};
  return w;
}

// The whole tile on the host; the estimates are added in pixel order.
inline double fold_host(size_t npix, const float* S, float* planes, const Fold& f) {
  F4* p = reinterpret_cast<F4*>(planes);
  double sse = 0.0;
  for (size_t i = 0; i < npix; ++i) sse += (double)fold_pixel(i, npix, S, p, f);
  return sse;
}

}  // namespace ptnz
