// pt_denoise.h — the edge-avoiding à-trous filter of include/pt_amd.h (pt_denoise), ONE implementation of its arithmetic.
//
// The per-pixel prepare / level / finish bodies below are what the HIP kernels (pt_denoise.hip) and the host loop
// (denoise_host, exported as pt_denoise_host) both run, so the two cannot disagree; tests/denoise_ref.py restates them in numpy.
// There is one body per step, and what a form (ptdn::Form) adds to it stands under `if constexpr`.  The variance-guided form
// (pt_denoise_guided; tests/denoise_guided_ref.py): the colour term is scaled by the centre's variance, which is prepared from the noise
// planes, prefiltered once and filtered along with the colour.  The adaptive form (pt_denoise_adaptive; tests/denoise_adaptive_ref.py)
// is the guided one with the sample counts of every pixel instead of two scalars in the prepare and the prefilter; its levels and its
// finish are the guided form's.  The history form (pt_history_denoise; tests/history_variance_ref.py) is the guided one over the blend
// of the image with the reprojected history (pt_history.h): its prepare takes the blend for the colour and the blend's variance for
// the variance; prefilter, levels and finish are the guided form's.  The moments form (pt_history_denoise_ex with PT_HISTORY_MOMENTS;
// tests/history_moments_ref.py) is the history form without a fold: its prepare takes the blend's variance from the moments the history
// carries (the differences between views), and marks the pixels whose history is too short; var_spatial_pixel — a step of its own
// between prepare and the prefilter — gives those the variance of their 7 x 7 neighbourhood instead.  The feedback form
// (pt_history_denoise_feedback; tests/history_feedback_ref.py) is the moments form over another colour: its prepare filters the blend of
// the new samples with the FILTERED history FC (pt_history.h), the variance still comes from the raw chain (or, by option, from the
// variance FC carries), and tap_pixel — a step of its own after level L - 1 — leaves {c_L remodulated, var_L}, the plane the next capture
// promotes to FK.  Everything between is the moments form's.  The history form with per-pixel counts (pt_history_denoise_adaptive;
// tests/history_threshold_ref.py) is the history form's prepare with the counts of every pixel (Tf_p, Df_p; the blend's samples are
// Tf_p) and NE_p = Tf_p + Th in the position buffer's spare word, followed by the adaptive form's prefilter, levels and finish.
// Every float operation is a separate IEEE operation in the order pt_amd.h states (`#pragma clang fp contract(off)` in every body, correctly
// rounded division, denormals kept), so the result does not depend on the arithmetic mode of the build or on the side it runs on.
// Plain C++ apart from PT_HD: the system compiler accepts it (a host sanitizer run needs nothing else).
//
// Mapping of a level: one thread filters kRows pixels of one column, rows y0, y0 + s, .., y0 + (kRows - 1) s —
// pixels of one residue class of the step's lattice, whose 5 x 5 stencils overlap in all but one row each.  The thread walks the
// kRows + 4 lattice rows once, loads every tap (colour, normal + hit flag, position: 3 x 16 B) once and feeds it to every centre
// within two lattice rows: 5 (kRows + 4) taps loaded for 25 kRows used (kRows = 4: 40 for 100), the same code at every step.  A
// centre still meets its taps rows outer, columns inner, so its sums are added in the stated order.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_adaptive.h"
#include "pt_history.h"
#include "pt_portable_math.h"

namespace ptdn {

struct alignas(16) V4 {
  float x, y, z, w;
};

constexpr int kRows = 4;        // pixels of one column per thread of a level (see above)
constexpr int kMaxLevels = 8;
constexpr int kWorkspaceV4 = 5;  // per pixel: normal + hit | position | albedo | colour ping | colour pong
static_assert(kWorkspaceV4 * sizeof(V4) == 80, "pt_amd.h documents 80 bytes of workspace per pixel");

struct Params {
  int levels;
  float inv_c, inv_n, inv_p;  // 1 / sigma^2 in float32; 0: the term is off
  int keep_albedo;
};

// PtDenoiseOptions -> Params (0 = the default in every field, NULL = all defaults); the message of a refusal, or nullptr.
// default_color: sigma_color's default, 4 for pt_denoise, kGuidedSigmaColor for the guided form.
constexpr float kGuidedSigmaColor = 8.0f;
constexpr float kHistorySigmaColor = 8.0f;  // the history form's
inline const char* resolve(const PtDenoiseOptions* opt, Params* out, float default_color = 4.0f) {
#pragma clang fp contract(off)
  PtDenoiseOptions o{};
  if (opt) o = *opt;
  if (o.levels == 0) o.levels = 5;
  if (o.levels < 1 || o.levels > kMaxLevels) return "levels outside 1 .. 8";
  const float sig[3] = {o.sigma_color, o.sigma_normal, o.sigma_position};
  const float def[3] = {default_color, 0.5f, 1.0f};
  float inv[3];
  for (int k = 0; k < 3; ++k) {
    if (!(sig[k] - sig[k] == 0.0f)) return "a sigma is not finite";
    const float s = sig[k] == 0.0f ? def[k] : sig[k];
    inv[k] = s < 0.0f ? 0.0f : 1.0f / (s * s);
  }
  if (o.keep_albedo != 0 && o.keep_albedo != 1) return "keep_albedo is 0 or 1";
  *out = Params{o.levels, inv[0], inv[1], inv[2], o.keep_albedo};
  return nullptr;
}
// The colour term's factor at level l: inv_c * 4^l (the noise left after l levels is that much smaller)
PT_HD float color_factor(const Params& P, int l) {
#pragma clang fp contract(off)
  return P.inv_c * (float)(1 << (2 * l));
}

// The three forms of the filter, and what a form divides by.  Plain: Tf, the samples.  Guided: ptnz::fold_scalars' Tf and Df of the folds so
// far.  Adaptive: the counts of the pixel itself — cnt, the plane of pt_adaptive.h, or nullptr: the uniform state, (T, M) for every
// pixel, as ptad::resolve_pixel.  History: the guided form's two for the new samples' variance, and what the blend reads — samples, the
// history's current plane C and its variance VC (both nullptr: absent).
// Moments: what the blend reads only — samples, C and VC = {m2h.xyz, rh} (both nullptr: absent); no fold, no noise planes.
// E (the moments form; nullptr: absent): the extra plane of the history round — the pixel's samples are samples + E_p (pthi::Counted).
// Feedback: the moments form's and FC = {f.xyz, vf} beside C (nullptr: absent), and the variance rule (PtHistoryFeedbackOptions.variance).
// HistoryAdaptive: the adaptive form's counts and the history form's C and VC; the blend's samples are the pixel's own Tf_p.
enum class Form { Plain, Guided, Adaptive, History, Moments, Feedback, HistoryAdaptive };
struct Divisors {
  float Tf, Df;
  const ptad::Cnt* cnt;
  int32_t T, M;
  float samples;
  const V4 *C, *VC;
  const float* E;
  const V4* FC;
  int fb_variance;
};
// A prepare's D has a member E: Divisors (the host loop, and a launch's checks) and the counted kernel's arguments; the kernels that
// existed before the history round take structs without one and are compiled as they were.
template <typename D, typename = void>
struct HasExtra : std::false_type {};
template <typename D>
struct HasExtra<D, std::void_t<decltype(std::declval<const D&>().E)>> : std::true_type {};
// The samples of pixel i as the history forms' prepare reads them
template <typename D>
PT_HD float history_samples(const D& d, size_t i) {
  if constexpr (HasExtra<D>::value) {
    if (d.E) return pthi::samples_of(pthi::Counted{d.samples, d.E}, i);
  }
  return d.samples;
}

// ── prepare: pixel i of the frame ────────────────────────────────────────────────────────────────────────────────────────
// guided: the fold's own estimate of one component (pt_noise.h fold_component's last two lines, on the planes it left), demodulated
// like the colour it belongs to
PT_HD float guided_variance(float prev, float q, float albedo, float Tf, float Df, int keep_albedo) {
#pragma clang fp contract(off)
  const float v = pthi::sample_variance(prev, q, Tf, Df);
  return !keep_albedo && albedo > 0.0f ? v / (albedo * albedo) : v;
}
// history: the variance of the blend of one component (pt_history.h blend_variance over the same estimate), demodulated likewise
PT_HD float history_variance(float prev, float q, float albedo, float Tf, float Df, float samples, float vh, float Th, int keep_albedo) {
#pragma clang fp contract(off)
  const float v = pthi::blend_variance(pthi::sample_variance(prev, q, Tf, Df), samples, vh, Th);
  return !keep_albedo && albedo > 0.0f ? v / (albedo * albedo) : v;
}
// moments: the unbiased variance of the weighted mean of the views from their second moment m2b and mean cb, f = rb / (1 - rb)
// (m2 - c^2 underestimates the per-view variance by (1 - r), and the blend's variance is r times that), demodulated likewise
PT_HD float moments_variance(float m2b, float cb, float f, float albedo, int keep_albedo) {
#pragma clang fp contract(off)
  const float d = m2b - cb * cb;
  const float v = (d > 0.0f ? d : 0.0f) * f;
  return !keep_albedo && albedo > 0.0f ? v / (albedo * albedo) : v;
}
// feedback, variance rule 1: the per-view variance of one component from the raw chain, s = d / (1 - rb) (g = 1 - rb), demodulated likewise
PT_HD float feedback_view_variance(float m2b, float cb, float g, float albedo, int keep_albedo) {
#pragma clang fp contract(off)
  const float d = m2b - cb * cb;
  const float s = (d > 0.0f ? d : 0.0f) / g;
  return !keep_albedo && albedo > 0.0f ? s / (albedo * albedo) : s;
}
// ... and what its prepare leaves in var_raw's place for a pixel whose history is too short to have one (every other var_raw is
// >= 0 or NaN: sums of clamped terms times f >= 0)
constexpr float kSpatialMark = -1.0f;
PT_HD bool spatial_marked(float var_raw) { return var_raw == kSpatialMark; }
// The guided forms (noise: the fold's two planes) leave var_raw in the albedo buffer's spare word.  The adaptive form leaves Tf_p in
// the position buffer's spare word, which no tap reads (dist2: xyz) and the other two leave 0; the history form with counts leaves
// NE_p = Tf_p + Th there.
// D: Divisors, or the members of it that the form reads (a kernel takes no more than those).
template <Form kForm, typename D>
PT_HD void prepare_pixel_of(size_t i, size_t npix, const float* S, const V4* planes, const V4* noise, const D& d, int keep_albedo, V4* n, V4* p, V4* a,
                            V4* c) {
#pragma clang fp contract(off)
  [[maybe_unused]] float Tf = 0.0f, Df = 0.0f;
  if constexpr (kForm == Form::Adaptive || kForm == Form::HistoryAdaptive) {
    const int32_t Tp = d.cnt ? d.cnt[i].T : d.T, Mp = d.cnt ? d.cnt[i].M : d.M;
    Tf = (float)Tp;
    Df = (float)(Mp - 1) * Tf;
  } else if constexpr (kForm != Form::Moments && kForm != Form::Feedback) {
    Tf = d.Tf;
    if constexpr (kForm == Form::Guided || kForm == Form::History) Df = d.Df;
  }
  const V4 s0 = planes[i], s1 = planes[npix + i], s2 = planes[2 * npix + i];
  const bool hit = s1.w > 0.0f;
  V4 vn{0.0f, 0.0f, 0.0f, hit ? 1.0f : 0.0f}, va{0.0f, 0.0f, 0.0f, 0.0f}, vp{0.0f, 0.0f, 0.0f, kForm == Form::Adaptive ? Tf : 0.0f};
  if (hit) {
    vn.x = s0.x / s1.w, vn.y = s0.y / s1.w, vn.z = s0.z / s1.w;
    va.x = s1.x / s1.w, va.y = s1.y / s1.w, va.z = s1.z / s1.w;
    vp.x = s2.x / s1.w, vp.y = s2.y / s1.w, vp.z = s2.z / s1.w;
  }
  V4 vc{0.0f, 0.0f, 0.0f, 0.0f};
  [[maybe_unused]] V4 hc{0.0f, 0.0f, 0.0f, 0.0f}, hv{0.0f, 0.0f, 0.0f, 0.0f};  // history: C and VC of the pixel (absent: +0)
  [[maybe_unused]] float ns = 0.0f;  // history: the pixel's samples (with its extras, where the history round left some)
  if constexpr (kForm == Form::History || kForm == Form::Moments || kForm == Form::Feedback || kForm == Form::HistoryAdaptive) {
    if constexpr (kForm == Form::HistoryAdaptive) ns = Tf;
    else ns = history_samples(d, i);
    if (d.C) hc = d.C[i];
    if (d.VC) hv = d.VC[i];
    vc.x = pthi::blend_component(S[3 * i], ns, hc.x, hc.w);
    vc.y = pthi::blend_component(S[3 * i + 1], ns, hc.y, hc.w);
    vc.z = pthi::blend_component(S[3 * i + 2], ns, hc.z, hc.w);
  } else {
    vc.x = S[3 * i] / Tf, vc.y = S[3 * i + 1] / Tf, vc.z = S[3 * i + 2] / Tf;
  }
  [[maybe_unused]] const V4 cb = vc;  // (moments: the blend before demodulation)
  if constexpr (kForm == Form::Feedback) {  // the colour that is filtered: the new samples with the FILTERED history, weighted as the raw blend
    const V4 hf = d.FC ? d.FC[i] : V4{0.0f, 0.0f, 0.0f, 0.0f};
    vc.x = pthi::blend_component(S[3 * i], ns, hf.x, hc.w);
    vc.y = pthi::blend_component(S[3 * i + 1], ns, hf.y, hc.w);
    vc.z = pthi::blend_component(S[3 * i + 2], ns, hf.z, hc.w);
  }
  if (!keep_albedo) {
    vc.x = va.x > 0.0f ? vc.x / va.x : vc.x;
    vc.y = va.y > 0.0f ? vc.y / va.y : vc.y;
    vc.z = va.z > 0.0f ? vc.z / va.z : vc.z;
  }
  if constexpr (kForm == Form::History || kForm == Form::HistoryAdaptive) {
    const V4 prev = noise[i], q = noise[npix + i];
    const float vx = history_variance(prev.x, q.x, va.x, Tf, Df, ns, hv.x, hc.w, keep_albedo);
    const float vy = history_variance(prev.y, q.y, va.y, Tf, Df, ns, hv.y, hc.w, keep_albedo);
    const float vz = history_variance(prev.z, q.z, va.z, Tf, Df, ns, hv.z, hc.w, keep_albedo);
    va.w = (vx + vy) + vz;
  } else if constexpr (kForm == Form::Moments || kForm == Form::Feedback) {
    const V4 mb = pthi::blend_moments(i, S, ns, hc.w, hv);
    if (mb.w <= PT_HISTORY_MOMENTS_R_MAX) {
      const float f = mb.w / (1.0f - mb.w);
      const float vx = moments_variance(mb.x, cb.x, f, va.x, keep_albedo);
      const float vy = moments_variance(mb.y, cb.y, f, va.y, keep_albedo);
      const float vz = moments_variance(mb.z, cb.z, f, va.z, keep_albedo);
      va.w = (vx + vy) + vz;
      if constexpr (kForm == Form::Feedback) {
        if (d.fb_variance) {  // rule 1 in its place: the new view's variance and the one the filtered history carries, weighted as the blend
          const float g = 1.0f - mb.w;
          const float sx = feedback_view_variance(mb.x, cb.x, g, va.x, keep_albedo);
          const float sy = feedback_view_variance(mb.y, cb.y, g, va.y, keep_albedo);
          const float sz = feedback_view_variance(mb.z, cb.z, g, va.z, keep_albedo);
          const float sv = (sx + sy) + sz;
          const pthi::MomentWeights w = pthi::moment_weights(ns, hc.w);
          va.w = (w.wn * w.wn) * sv + (w.wh * w.wh) * (d.FC ? d.FC[i].w : 0.0f);
        }
      }
    } else {
      va.w = kSpatialMark;  // too few views behind the blend (C absent included): var_spatial_pixel
    }
  } else if constexpr (kForm != Form::Plain) {
    const V4 prev = noise[i], q = noise[npix + i];
    const float vx = guided_variance(prev.x, q.x, va.x, Tf, Df, keep_albedo);
    const float vy = guided_variance(prev.y, q.y, va.y, Tf, Df, keep_albedo);
    const float vz = guided_variance(prev.z, q.z, va.z, Tf, Df, keep_albedo);
    va.w = (vx + vy) + vz;
  }
  if constexpr (kForm == Form::HistoryAdaptive) vp.w = Tf + hc.w;  // NE_p, the blend's effective sample count: what the prefilter scales by
  n[i] = vn, p[i] = vp, a[i] = va, c[i] = vc;
}

// The squared distance of two colours, normals or positions (xyz)
PT_HD float dist2(const V4& q, const V4& o) {
#pragma clang fp contract(off)
  const float dx = q.x - o.x, dy = q.y - o.y, dz = q.z - o.z;
  return (dx * dx + dy * dy) + dz * dz;
}

// moments, the spatial estimate: a marked pixel (x, y) takes var_raw from the DEMODULATED colours c of its 7 x 7 neighbourhood on its
// own side of hit / miss, weighted by the level's normal and position terms (no colour term, no H): the weighted variance of the
// neighbours, per channel, summed.  Reads c, n, p of the taps (3 x 16 B each), writes the centre's own spare word a.w only and reads
// no neighbour's, so the update in place has no hazard.  The centre tap passes with w = 1: wsum >= 1.
constexpr int kSpatialRadius = 3;
PT_HD void var_spatial_pixel(int W, int R, int x, int y, const Params& P, const V4* n, const V4* p, const V4* c, V4* a) {
#pragma clang fp contract(off)
  const size_t i0 = (size_t)y * W + x;
  const V4 cn = n[i0], cp = p[i0];
  float wsum = 0.0f, s1x = 0.0f, s1y = 0.0f, s1z = 0.0f, s2x = 0.0f, s2y = 0.0f, s2z = 0.0f;
  for (int j = -kSpatialRadius; j <= kSpatialRadius; ++j) {
    const int yt = y + j;
    if (yt < 0 || yt >= R) continue;
    for (int i = -kSpatialRadius; i <= kSpatialRadius; ++i) {
      const int xt = x + i;
      if (xt < 0 || xt >= W) continue;
      const size_t q = (size_t)yt * W + xt;
      const V4 qn = n[q];
      if (qn.w != cn.w) continue;
      const V4 qp = p[q], qc = c[q];
      const float dn = dist2(qn, cn), dp = dist2(qp, cp);
      const float e = dn * P.inv_n + dp * P.inv_p;
      const float w = ptmath::exp32(-e);
      wsum = wsum + w;
      s1x = s1x + w * qc.x, s1y = s1y + w * qc.y, s1z = s1z + w * qc.z;
      s2x = s2x + w * (qc.x * qc.x), s2y = s2y + w * (qc.y * qc.y), s2z = s2z + w * (qc.z * qc.z);
    }
  }
  const float mx = s1x / wsum, my = s1y / wsum, mz = s1z / wsum;
  float dx = s2x / wsum - mx * mx, dy = s2y / wsum - my * my, dz = s2z / wsum - mz * mz;
  dx = dx > 0.0f ? dx : 0.0f, dy = dy > 0.0f ? dy : 0.0f, dz = dz > 0.0f ? dz : 0.0f;
  a[i0].w = (dx + dy) + dz;
}

// guided variance prefilter: pixel (x, y); 3 x 3, binomial, over the pixels on the centre's side of hit / miss.  Reads the hit flags
// and var_raw (a.w), writes var_0 into the spare word of colour buffer 0 (4 bytes each: 24 B per pixel with the eight neighbours in cache).
// kAdaptive: over the per-sample variance var_raw(q) * Tf_q (p.w; neighbours differ in their counts: the selection key's argument and
// arithmetic, ptad::key_pixel), back in the centre's unit.
template <bool kAdaptive>
PT_HD void var_prefilter_of(int W, int R, int x, int y, const V4* n, const V4* a, const V4* p, V4* c0) {
#pragma clang fp contract(off)
  constexpr float G[3] = {1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f};
  const size_t i0 = (size_t)y * W + x;
  const float hit = n[i0].w;
  float acc = 0.0f, gsum = 0.0f;
#pragma unroll
  for (int j = -1; j <= 1; ++j) {
    const int yt = y + j;
    if (yt < 0 || yt >= R) continue;
#pragma unroll
    for (int i = -1; i <= 1; ++i) {
      const int xt = x + i;
      if (xt < 0 || xt >= W) continue;
      const size_t q = (size_t)yt * W + xt;
      if (n[q].w != hit) continue;
      const float g = G[j + 1] * G[i + 1];
      float s = a[q].w;
      if constexpr (kAdaptive) s = s * p[q].w;
      acc = acc + g * s;
      gsum = gsum + g;
    }
  }
  float v = acc / gsum;
  if constexpr (kAdaptive) v = v / p[i0].w;
  c0[i0].w = v;
}

// ── level: one tap against one centre ────────────────────────────────────────────────────────────────────────────────────
struct Centre {
  V4 c, n, p;  // n.w: the hit flag (1 / 0), or -1: no such pixel (no tap matches it)
  float ax, ay, az, wsum;
};
// guided: the centre carries its own colour factor (set once from its variance) and the sum of w^2 var(q); qc.w is var_l(q)
struct CentreGuided : Centre {
  float cf, vsum;
};
template <bool kGuided>
using CentreOf = typename std::conditional<kGuided, CentreGuided, Centre>::type;
PT_HD float guided_color_factor(const Params& P, float var) {
#pragma clang fp contract(off)
  return P.inv_c / (var + PT_DENOISE_VARIANCE_FLOOR);
}
// cf: the level's colour factor, which the guided form replaces with the centre's own
template <bool kGuided>
PT_HD void tap_of(CentreOf<kGuided>& ce, float h, float cf, const Params& P, const V4& qc, const V4& qn, const V4& qp) {
#pragma clang fp contract(off)
  if (qn.w != ce.n.w) return;
  if constexpr (kGuided) cf = ce.cf;
  const float dc = dist2(qc, ce.c), dn = dist2(qn, ce.n), dp = dist2(qp, ce.p);
  const float e = (dc * cf + dn * P.inv_n) + dp * P.inv_p;
  const float w = h * ptmath::exp32(-e);
  ce.ax = ce.ax + w * qc.x;
  ce.ay = ce.ay + w * qc.y;
  ce.az = ce.az + w * qc.z;
  ce.wsum = ce.wsum + w;
  if constexpr (kGuided) ce.vsum = ce.vsum + (w * w) * qc.w;
}

// Threads of a level over a frame of R rows: column x, row slot ty < level_slots(R, l); slot ty filters the rows
// first_row(ty, l) + k * s, k < kRows, that exist.  (Groups of kRows * s rows, one slot per residue of the step.)
PT_HD int level_slots(int R, int l) {
  const int span = kRows << l;
  return ((R + span - 1) / span) << l;
}
PT_HD int first_row(int ty, int l) { return (ty >> l) * (kRows << l) + (ty & ((1 << l) - 1)); }

// Level l for the pixels of column x in slot ty: reads c, n, p, writes `out` (the other colour buffer).  kGuided: c.w is the variance
// that belongs to c.xyz, and out.w the variance of what is written.
template <bool kGuided>
PT_HD void level_column_of(int W, int R, int x, int ty, int l, const Params& P, const V4* c, const V4* n, const V4* p, V4* out) {
#pragma clang fp contract(off)
  constexpr float H[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
  const int s = 1 << l;
  const int y0 = first_row(ty, l);
  if (y0 >= R) return;  // (a slot of the last, partial group of rows)
  const float cf = kGuided ? 0.0f : color_factor(P, l);
  CentreOf<kGuided> ce[kRows];
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int y = y0 + k * s;
    ce[k].ax = ce[k].ay = ce[k].az = ce[k].wsum = 0.0f;
    if (y < R) {
      const size_t q = (size_t)y * W + x;
      ce[k].c = c[q], ce[k].n = n[q], ce[k].p = p[q];
    } else {
      ce[k].c = ce[k].p = V4{0.0f, 0.0f, 0.0f, 0.0f};
      ce[k].n = V4{0.0f, 0.0f, 0.0f, -1.0f};
    }
    if constexpr (kGuided) ce[k].cf = guided_color_factor(P, ce[k].c.w), ce[k].vsum = 0.0f;
  }
#pragma unroll
  for (int m = 0; m < kRows + 4; ++m) {  // lattice row m - 2 relative to y0: the tap row j = m - 2 - k of centre k
    const int yt = y0 + (m - 2) * s;
    if (yt < 0 || yt >= R) continue;
#pragma unroll
    for (int i = -2; i <= 2; ++i) {
      const int xt = x + i * s;
      if (xt < 0 || xt >= W) continue;
      const size_t q = (size_t)yt * W + xt;
      const V4 qc = c[q], qn = n[q], qp = p[q];
#pragma unroll
      for (int k = 0; k < kRows; ++k) {
        const int j = m - 2 - k;
        if (j >= -2 && j <= 2) tap_of<kGuided>(ce[k], H[j + 2] * H[i + 2], cf, P, qc, qn, qp);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int y = y0 + k * s;
    if (y >= R) continue;
    float var = 0.0f;
    if constexpr (kGuided) var = ce[k].vsum / (ce[k].wsum * ce[k].wsum);
    out[(size_t)y * W + x] = V4{ce[k].ax / ce[k].wsum, ce[k].ay / ce[k].wsum, ce[k].az / ce[k].wsum, var};
  }
}

// ── finish: pixel i ──────────────────────────────────────────────────────────────────────────────────────────────────────
PT_HD void finish_pixel(size_t i, int keep_albedo, const V4* c, const V4* a, float* out) {
#pragma clang fp contract(off)
  const V4 vc = c[i], va = a[i];
  const bool demod = !keep_albedo;
  out[3 * i] = demod && va.x > 0.0f ? vc.x * va.x : vc.x;
  out[3 * i + 1] = demod && va.y > 0.0f ? vc.y * va.y : vc.y;
  out[3 * i + 2] = demod && va.z > 0.0f ? vc.z * va.z : vc.z;
}

// feedback, the tap: pixel i of the pending plane P = {c_L remodulated as the finish step does, var_L}.  P4: a device plane (16-byte
// stores) or a caller's host array (pthi::F4)
template <typename P4>
PT_HD void tap_pixel(size_t i, int keep_albedo, const V4* c, const V4* a, P4* tap) {
#pragma clang fp contract(off)
  const V4 vc = c[i], va = a[i];
  const bool demod = !keep_albedo;
  tap[i] = P4{demod && va.x > 0.0f ? vc.x * va.x : vc.x, demod && va.y > 0.0f ? vc.y * va.y : vc.y, demod && va.z > 0.0f ? vc.z * va.z : vc.z, vc.w};
}

// The colour buffer that holds c_l (prepare writes c_0 into buffer 0, level l reads l & 1 and writes the other); the finish step
// writes its 12 bytes per pixel over the buffer that does not hold c_levels.
PT_HD int color_buffer(int l) { return l & 1; }

// What a launch or the host loop filters: the frame and its arrays (noise: the fold's PT_NOISE_PLANES planes, null for the plain form),
// and the resolved divisors and parameters.  pt_denoise_launch reads device pointers, denoise_host the caller's arrays.
// current, current_var (the history form; both null: absent): the planes C and VC, which the host loop reads here and a launch in div.
struct Frame {
  int w, rows;
  const float *rgb_sum, *planes, *noise;
  const float *current = nullptr, *current_var = nullptr;
  const float* extra = nullptr;  // the moments form: the extra plane E, w * rows floats (null: absent)
  const float* feedback = nullptr;  // the feedback form: the plane FC beside `current` (null: absent), which the host loop reads here
};
// tap_level, tap (the feedback form): after level tap_level - 1 the plane `tap` (w * rows float4: a device plane for a launch, a
// caller's array for the host loop) receives tap_pixel of c_(tap_level); 1 .. P.levels.
struct Job {
  Form form;
  Frame f;
  Divisors div;
  Params P;
  int tap_level = 0;
  void* tap = nullptr;
};

// The whole filter on the host, with the bodies above in the kernels' own thread order.  counts (the adaptive form): {T_p, M_p} per pixel
// (pt_readback_adaptive's layout), every M_p >= 2 and T_p >= M_p.  var_raw / var_0 (npix floats each, or null; the two guided forms)
// receive the prepared and the prefiltered variance; out may then be null.  The moments form: var_raw is what the spatial step left,
// and mark (npix bytes, or null) receives 1 for the pixels prepare marked for it, 0 for the others.
inline void denoise_host(const Job& j, const int32_t* counts, float* out, float* var_raw = nullptr, float* var_0 = nullptr, uint8_t* mark = nullptr) {
  const int W = j.f.w, R = j.f.rows;
  const Params& P = j.P;
  const bool feedback = j.form == Form::Feedback, moments = j.form == Form::Moments || feedback;
  const bool counted = j.form == Form::Adaptive || j.form == Form::HistoryAdaptive;
  const bool guided = j.form != Form::Plain, folded = guided && !moments, blended = j.form == Form::History || j.form == Form::HistoryAdaptive || moments;
  const size_t npix = (size_t)W * R;
  std::vector<V4> ws(kWorkspaceV4 * npix);
  V4 *n = ws.data(), *p = n + npix, *a = p + npix, *col[2] = {a + npix, a + 2 * npix};
  std::vector<V4> pl((PT_FEATURE_PLANES + (folded ? PT_NOISE_PLANES : 0)) * npix);  // (the caller's planes need not be 16-byte aligned)
  V4* nz = pl.data() + PT_FEATURE_PLANES * npix;
  for (size_t i = 0; i < PT_FEATURE_PLANES * npix; ++i) pl[i] = V4{j.f.planes[4 * i], j.f.planes[4 * i + 1], j.f.planes[4 * i + 2], j.f.planes[4 * i + 3]};
  for (size_t i = 0; i < PT_NOISE_PLANES * npix && folded; ++i) nz[i] = V4{j.f.noise[4 * i], j.f.noise[4 * i + 1], j.f.noise[4 * i + 2], j.f.noise[4 * i + 3]};
  std::vector<ptad::Cnt> cnt(counts ? npix : 0);
  for (size_t i = 0; i < cnt.size(); ++i) cnt[i] = ptad::Cnt{counts[2 * i], counts[2 * i + 1]};
  Divisors d = j.div;
  if (counts) d.cnt = cnt.data();
  std::vector<V4> hist(blended && j.f.current ? 2 * npix : 0);
  for (size_t i = 0; i < hist.size() / 2; ++i) {
    const float *c = j.f.current + 4 * i, *v = j.f.current_var + 4 * i;
    hist[i] = V4{c[0], c[1], c[2], c[3]}, hist[npix + i] = V4{v[0], v[1], v[2], v[3]};
  }
  if (blended) d.C = hist.empty() ? nullptr : hist.data(), d.VC = hist.empty() ? nullptr : hist.data() + npix;
  std::vector<V4> fbc(feedback && j.f.feedback ? npix : 0);
  for (size_t i = 0; i < fbc.size(); ++i) fbc[i] = V4{j.f.feedback[4 * i], j.f.feedback[4 * i + 1], j.f.feedback[4 * i + 2], j.f.feedback[4 * i + 3]};
  d.FC = fbc.empty() ? nullptr : fbc.data();
  d.E = moments ? j.f.extra : nullptr;
  for (size_t i = 0; i < npix; ++i) {
    if (j.form == Form::Plain) prepare_pixel_of<Form::Plain>(i, npix, j.f.rgb_sum, pl.data(), nz, d, P.keep_albedo, n, p, a, col[0]);
    else if (j.form == Form::Guided) prepare_pixel_of<Form::Guided>(i, npix, j.f.rgb_sum, pl.data(), nz, d, P.keep_albedo, n, p, a, col[0]);
    else if (j.form == Form::History) prepare_pixel_of<Form::History>(i, npix, j.f.rgb_sum, pl.data(), nz, d, P.keep_albedo, n, p, a, col[0]);
    else if (j.form == Form::Moments) prepare_pixel_of<Form::Moments>(i, npix, j.f.rgb_sum, pl.data(), nullptr, d, P.keep_albedo, n, p, a, col[0]);
    else if (feedback) prepare_pixel_of<Form::Feedback>(i, npix, j.f.rgb_sum, pl.data(), nullptr, d, P.keep_albedo, n, p, a, col[0]);
    else if (j.form == Form::HistoryAdaptive) prepare_pixel_of<Form::HistoryAdaptive>(i, npix, j.f.rgb_sum, pl.data(), nz, d, P.keep_albedo, n, p, a, col[0]);
    else prepare_pixel_of<Form::Adaptive>(i, npix, j.f.rgb_sum, pl.data(), nz, d, P.keep_albedo, n, p, a, col[0]);
  }
  for (size_t i = 0; i < npix && mark; ++i) mark[i] = moments && spatial_marked(a[i].w) ? 1 : 0;
  for (int y = 0; y < R && moments; ++y)
    for (int x = 0; x < W; ++x)
      if (spatial_marked(a[(size_t)y * W + x].w)) var_spatial_pixel(W, R, x, y, P, n, p, col[0], a);
  for (int y = 0; y < R && guided; ++y)
    for (int x = 0; x < W; ++x) {
      if (counted) var_prefilter_of<true>(W, R, x, y, n, a, p, col[0]);
      else var_prefilter_of<false>(W, R, x, y, n, a, p, col[0]);
    }
  for (size_t i = 0; i < npix && var_raw; ++i) var_raw[i] = a[i].w;
  for (size_t i = 0; i < npix && var_0; ++i) var_0[i] = col[0][i].w;
  const bool tapped = feedback && j.tap;
  if (!out && !tapped) return;
  for (int l = 0; l < P.levels; ++l) {
    for (int ty = 0; ty < level_slots(R, l); ++ty)
      for (int x = 0; x < W; ++x) {
        if (guided) level_column_of<true>(W, R, x, ty, l, P, col[color_buffer(l)], n, p, col[color_buffer(l + 1)]);
        else level_column_of<false>(W, R, x, ty, l, P, col[color_buffer(l)], n, p, col[color_buffer(l + 1)]);
      }
    for (size_t i = 0; i < npix && tapped && l + 1 == j.tap_level; ++i) tap_pixel(i, P.keep_albedo, col[color_buffer(l + 1)], a, static_cast<pthi::F4*>(j.tap));
  }
  for (size_t i = 0; i < npix && out; ++i) finish_pixel(i, P.keep_albedo, col[color_buffer(P.levels)], a, out);
}

}  // namespace ptdn
