// pt_adaptive.h — adaptive sampling (include/pt_amd.h pt_adaptive_round), ONE implementation of its arithmetic.
//
// key_pixel, merge_pixel and resolve_pixel below are what the HIP kernels (pt_adaptive.hip) and the host loops (exported as
// pt_adaptive_select_host / pt_adaptive_merge_host) both run, so the two cannot disagree; tests/adaptive_ref.py restates them in
// numpy.  Every float operation is a separate IEEE operation in the order pt_amd.h states (`#pragma clang fp contract(off)`,
// correctly rounded division, denormals kept), as in pt_noise.h, whose planes (prev.xyz | w, q.xyz | 0) these functions read and write.
// Plain C++ apart from PT_HD.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_noise.h"
#include "pt_portable_math.h"

namespace ptad {

struct Cnt {  // the plane `cnt`: iterations and groups of ONE pixel
  int32_t T, M;
};
static_assert(sizeof(Cnt) == 8, "pt_amd.h documents 8 bytes per pixel");

PT_HD uint32_t key_bits(float key) {
  return key != key ? 0xffffffffu : __builtin_bit_cast(uint32_t, key);  // a NaN sorts first, whatever its sign and payload
}

// The selection key of pixel (x, y) of a tile of W x R pixels: the 3x3 binomial prefilter of the per-sample variance s = w * T,
// back in the unit of w.  plane0 = the first noise plane (any type with a float member w), cnt = the count plane (any type with an
// int32 member T: pt_group_select.h reads both from one packed plane).
template <typename P4, typename C>
PT_HD uint32_t key_pixel(int x, int y, int W, int R, const P4* plane0, const C* cnt) {
#pragma clang fp contract(off)
  float num = 0.0f, den = 0.0f;
  for (int j = -1; j <= 1; ++j) {
    const int yy = y + j;
    if (yy < 0 || yy >= R) continue;
    for (int i = -1; i <= 1; ++i) {
      const int xx = x + i;
      if (xx < 0 || xx >= W) continue;
      const size_t q = (size_t)yy * W + xx;
      const float g = (j == 0 ? 0.5f : 0.25f) * (i == 0 ? 0.5f : 0.25f);  // G[j + 1] * G[i + 1], G = 1/4 1/2 1/4
      const float s = plane0[q].w * (float)cnt[q].T;
      num = num + g * s;
      den = den + g;
    }
  }
  const float f = num / den;
  return key_bits(f / (float)cnt[(size_t)y * W + x].T);
}

// One colour component of a merge: the group sum b joins S and q; returns the variance estimate of the average (the fold's v).
PT_HD float merge_component(float b, float* S, float* q, float nf, float Tf, float Df) {
#pragma clang fp contract(off)
  const float s = *S + b;
  *S = s;
  *q = *q + (b * b) / nf;
  const float d = *q - (s * s) / Tf;
  return (d > 0.0f ? d : 0.0f) / Df;
}
// List entry i of a merge: the worker's group sum Sw[i] of nf = (float)G iterations joins tile pixel p = list[i]; the pixel's new
// estimate w is in planes[p].w afterwards.
template <typename P4>
PT_HD void merge_pixel(size_t i, size_t npix, const int32_t* list, const float* Sw, float nf, int group_iters, float* S, P4* planes, Cnt* cnt) {
#pragma clang fp contract(off)
  const size_t p = (size_t)list[i];
  Cnt c = cnt[p];
  c.T += group_iters;
  c.M += 1;
  const float Tf = (float)c.T;
  const float Df = (float)(c.M - 1) * Tf;
  P4 q = planes[npix + p];
  float sx = S[3 * p], sy = S[3 * p + 1], sz = S[3 * p + 2];
  const float vx = merge_component(Sw[3 * i], &sx, &q.x, nf, Tf, Df);
  const float vy = merge_component(Sw[3 * i + 1], &sy, &q.y, nf, Tf, Df);
  const float vz = merge_component(Sw[3 * i + 2], &sz, &q.z, nf, Tf, Df);
  const float w = (vx + vy) + vz;
  S[3 * p] = sx, S[3 * p + 1] = sy, S[3 * p + 2] = sz;
  planes[p] = P4{sx, sy, sz, w};
  planes[npix + p] = P4{q.x, q.y, q.z, 0.0f};
  cnt[p] = c;
}

// Averaged radiance of pixel p: S / (float)T_p per component; cnt == nullptr: the uniform state, T_p = T for every pixel.
PT_HD void resolve_pixel(size_t p, const float* S, const Cnt* cnt, int32_t T, float* out) {
#pragma clang fp contract(off)
  const float Tf = (float)(cnt ? cnt[p].T : T);
  out[3 * p] = S[3 * p] / Tf;
  out[3 * p + 1] = S[3 * p + 1] / Tf;
  out[3 * p + 2] = S[3 * p + 2] / Tf;
}

inline int list_length(double fraction, int64_t npix) {
  const double want = std::ceil(fraction * (double)npix);
  return (int)std::min<double>((double)npix, std::max(1.0, want));
}

// Selection by threshold (pt_amd.h pt_adaptive_round_threshold): the key bits a pixel must EXCEED, thr = threshold * threshold in
// one float32 multiply (threshold finite and >= 0, so thr is never a NaN and its bits order like the float).
PT_HD uint32_t threshold_bits(float threshold) {
#pragma clang fp contract(off)
  const float thr = threshold * threshold;
  return __builtin_bit_cast(uint32_t, thr);
}
PT_HD bool above_threshold(uint32_t key, uint32_t thr) { return key > thr; }  // equal is not above; a NaN key (all bits set) is
// The cut (tau, r) of the top-`cap` selection — tau the cap-th largest key, r the pixels equal to it to take — under the threshold:
// while tau lies above thr the top `cap` are all above and the cut stands; otherwise every pixel above thr is taken and no tie.
struct Cut {
  uint32_t tau, r;
};
PT_HD Cut threshold_cut(uint32_t tau, uint32_t r, uint32_t thr) { return above_threshold(tau, thr) ? Cut{tau, r} : Cut{thr, 0u}; }
PT_HD uint32_t threshold_length(uint32_t above, uint32_t cap) { return above < cap ? above : cap; }  // m

inline std::vector<uint32_t> keys_host(int W, int R, const float* noise_planes, const int32_t* counts) {
  const ptnz::F4* plane0 = reinterpret_cast<const ptnz::F4*>(noise_planes);
  const Cnt* cnt = reinterpret_cast<const Cnt*>(counts);
  std::vector<uint32_t> key((size_t)W * R);
  for (int y = 0; y < R; ++y)
    for (int x = 0; x < W; ++x) key[(size_t)y * W + x] = key_pixel(x, y, W, R, plane0, cnt);
  return key;
}
// The cut of the top-m selection: the m-th largest key and the pixels equal to it that belong to the m.
inline Cut cut_host(const std::vector<uint32_t>& key, int m) {
  std::vector<uint32_t> sorted(key);
  std::nth_element(sorted.begin(), sorted.begin() + (m - 1), sorted.end(), [](uint32_t a, uint32_t b) { return a > b; });
  const uint32_t tau = sorted[(size_t)m - 1];
  size_t above = 0;
  for (uint32_t k : key) above += k > tau ? 1 : 0;
  return Cut{tau, (uint32_t)((size_t)m - above)};
}
// The pixels above the cut and the first r equal to it, in tile order; returns how many.
inline size_t scatter_host(const std::vector<uint32_t>& key, Cut c, int32_t* list) {
  size_t ties = c.r, out = 0;
  for (size_t p = 0; p < key.size(); ++p) {
    if (key[p] > c.tau) list[out++] = (int32_t)p;
    else if (key[p] == c.tau && ties > 0) list[out++] = (int32_t)p, --ties;
  }
  return out;
}

// The whole selection on the host: the m pixels with the largest key, equal keys by the smaller tile index, in ascending tile index.
inline void select_host(int W, int R, const float* noise_planes, const int32_t* counts, int m, int32_t* list) {
  const std::vector<uint32_t> key = keys_host(W, R, noise_planes, counts);
  scatter_host(key, cut_host(key, m), list);
}

// Selection by threshold on the host: *above = pixels whose key exceeds thr, *m = min(above, cap); list receives the m of them with
// the largest keys (ties by the smaller tile index) in ascending tile index.  The steps are the device's: cut for rank cap, clamp, scatter.
inline void select_threshold_host(int W, int R, const float* noise_planes, const int32_t* counts, float threshold, int cap, int32_t* list,
                                  int* above, int* m) {
  const std::vector<uint32_t> key = keys_host(W, R, noise_planes, counts);
  const uint32_t thr = threshold_bits(threshold);
  const Cut top = cut_host(key, cap);
  uint32_t n_above = 0;
  for (uint32_t k : key) n_above += above_threshold(k, thr) ? 1u : 0u;
  const size_t wrote = scatter_host(key, threshold_cut(top.tau, top.r, thr), list);
  *above = (int)n_above;
  *m = (int)threshold_length(n_above, (uint32_t)cap);
  (void)wrote;  // == *m
}

// A merge on the host; the estimates of ALL tile pixels are added in pixel order.
inline double merge_host(size_t npix, float* S, float* planes, int32_t* counts, const int32_t* list, int m, const float* Sw, int group_iters) {
  ptnz::F4* p4 = reinterpret_cast<ptnz::F4*>(planes);
  Cnt* cnt = reinterpret_cast<Cnt*>(counts);
  for (int i = 0; i < m; ++i) merge_pixel((size_t)i, npix, list, Sw, (float)group_iters, group_iters, S, p4, cnt);
  double sse = 0.0;
  for (size_t p = 0; p < npix; ++p) sse += (double)p4[p].w;
  return sse;
}

}  // namespace ptad
