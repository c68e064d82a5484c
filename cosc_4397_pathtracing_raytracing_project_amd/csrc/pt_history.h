// pt_history.h — the reprojected sample history of include/pt_amd.h (pt_history_capture / _reproject / _resolve), ONE implementation
// of its arithmetic.
//
// capture_pixel, reproject_pixel and blend_pixel below are what the HIP kernels (pt_history.hip) and the host loops (exported as
// pt_history_*_host) both run, so the two cannot disagree; tests/history_ref.py restates them in numpy.  Every float operation is a
// separate IEEE operation in the order pt_amd.h states (`#pragma clang fp contract(off)` in every body, correctly rounded division,
// denormals kept), so the planes do not depend on the arithmetic mode of the build or on the side they are computed on.  Plain C++
// apart from PT_HD.
//
//
// The variance side (PT_HISTORY_VARIANCE; capture_pixel_of<true>, reproject_pixel_of<true>): two more planes, VK = the per-channel
// variance of K0.xyz and VC = VK resampled beside C, so that the blend has a variance the guided filter can follow
// (pt_history_denoise: ptdn::Form::History in pt_denoise.h, whose prepare runs blend_component and blend_variance below).  The
// <false> instantiations are the bodies as they stood before the variance side existed.
//
// The moments side (PT_HISTORY_MOMENTS; capture_pixel_of<kMoments>, and the same reproject_pixel_of<true>): the two planes hold
// VK = {m2.xyz, r} instead — the second moment of the views' mean colours that formed K0.xyz, weighted as the colour was, and the sum
// of the squared weights of those views — so that the variance of the blend comes from the differences BETWEEN views and a view
// needs no fold (1 spp per view).  Its lookup interpolates all four components of VK where the variance kind's interpolates three and
// writes +0: reproject_pixel_of<kMoments>, an instantiation of its own, so that the variance kind's kernel is the code it was.
// pt_history_denoise_ex: ptdn::Form::Moments in pt_denoise.h, whose prepare runs blend_moments below.
//
// The history round (pt_history_round; round_key, merge_entry and Counted below): pixels whose carried weight Th is below min_history
// get a group of further iterations, for those pixels alone — the key orders them, pt_adaptive.h's selection lists them, the adaptive
// rounds' worker renders them, and the merge counts them in the extra plane E.  While E is present the blend, the capture and the
// moments read ns = samples + E_p where they read `samples`: the Counted instantiations, beside the ones that take a float and are
// the bodies as they stood.
//
// The history probes (pt_history_probe_keep / _check; probe_grid, probe_keep, probe_gradient and probe_apply below): a sparse grid of
// last view's sums, rendered again after an object moved — a sample is a pure function of (iteration, pixel, world), so the two sums
// differ exactly where a path met something that changed — and C.w shortened around the probes that differ.
//
// The feedback (PT_HISTORY_FEEDBACK; reproject_pixel_of<kMoments, .., true>): a parallel plane pair for the FILTERED colour, FK = {f.xyz, vf}
// beside K and FC beside C, resampled with the weights of the colour.  K0, VK, C and VC — the raw chain — are the bits they are
// without it: the moments' variance m2b - cb^2 needs the raw first moment.  pt_history_denoise_feedback: ptdn::Form::Feedback in
// pt_denoise.h, whose prepare filters blend(S, ns, FC, C.w) and whose tap leaves the plane the next capture promotes to FK.
//
// The noise estimate of the blend (pt_history_noise, pt_history_render_until; noise_value and noise_pixel below): the blend's variance of
// the variance side, summed over the channels per pixel — what pt_noise.hip's k_history_noise and k_noise_fold_history sum over the tile
// the way the fold sums its own estimate.
//
// Out of scope (pt_amd.h says the same): pt_group_* (a context's interleaved rows cannot look up their neighbours), feeding the
// moments into the noise estimate of the blend (noise_value below: the variance kind only), the history round in groups of contexts, a key of that round that uses the carried variance (threshold rounds keyed by the blend's variance: further down), objects that are added, removed or deformed (rigid and affine motion of an object: PT_HISTORY_MOTION), and correcting the smoothing the bilinear lookup adds — the carried image is a biased estimator, and the carried
// variance is interpolated linearly (as SVGF interpolates its moments), which overstates it: the lookup's smoothing lowers the true one.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/pt_amd.h"
#include "pt_adaptive.h"
#include "pt_portable_math.h"

namespace pthi {

struct alignas(16) V4 {  // the device's planes: one 16-byte load or store per pixel and plane
  float x, y, z, w;
};
struct F4 {  // a caller's host array of floats promises no more than float alignment
  float x, y, z, w;
};
constexpr int kKeptPlanes = PT_HISTORY_KEPT_PLANES;  // K0 colour | weight, K1 position | id, K2 normal | 0
constexpr int kPlanes = kKeptPlanes + 1;             // ... and the current plane C
static_assert(kPlanes * sizeof(V4) == 64, "pt_amd.h documents 64 bytes of state per pixel");
constexpr int kVarPlanes = 2;  // the variance state, a buffer of its own: VK beside K0, VC beside C
static_assert(kVarPlanes * sizeof(V4) == 32, "pt_amd.h documents 32 bytes of variance state per pixel");
constexpr float kMinWeight = 0.015625f;  // a lookup with less bilinear weight than 1/64 left carries nothing

// PtHistoryOptions with the defaults filled in.  A test that is switched off keeps its flag, not a sentinel value, so that the
// comparison it would make is not made at all.
struct Params {
  float cap, min_dot, plane_tol;
  int use_dot, use_plane, keep_view_dependent;
};
// 0 = the default in every field, NULL = all defaults; the message of a refusal, or nullptr.
inline const char* resolve(const PtHistoryOptions* opt, Params* out) {
  PtHistoryOptions o{};
  if (opt) o = *opt;
  if (!(o.cap - o.cap == 0.0f) || !(o.min_normal_dot - o.min_normal_dot == 0.0f) || !(o.plane_tol - o.plane_tol == 0.0f)) return "an option is not finite";
  if (o.cap == 0.0f) o.cap = 32.0f;
  if (!(o.cap > 0.0f)) return "cap must be positive";
  if (o.min_normal_dot == 0.0f) o.min_normal_dot = 0.9f;
  if (o.plane_tol == 0.0f) o.plane_tol = 0.02f;
  if (o.keep_view_dependent != 0 && o.keep_view_dependent != 1) return "keep_view_dependent is 0 or 1";
  *out = Params{o.cap, o.min_normal_dot, o.plane_tol, o.min_normal_dot < 0.0f ? 0 : 1, o.plane_tol < 0.0f ? 0 : 1, o.keep_view_dependent};
  return nullptr;
}

// The kept camera as the lookup reads it, and the tile it looks into: W x R pixels starting at frame row row0.
struct View {
  float pos[3], view[3], up[3], right[3];
  float plx, ply, hw, hh, wmax, hmax;  // wmax = (float)(W - 1), hmax = (float)(H - 1)
  int W, R, row0;
};
inline View make_view(const PtCamera& cam, int rows, int row0) {
#pragma clang fp contract(off)
  View v{};
  for (int k = 0; k < 3; ++k) v.pos[k] = cam.position[k], v.view[k] = cam.view[k], v.up[k] = cam.up[k], v.right[k] = cam.right[k];
  v.plx = cam.pixelLength[0], v.ply = cam.pixelLength[1];
  v.hw = (float)cam.resolution[0] * 0.5f, v.hh = (float)cam.resolution[1] * 0.5f;
  v.wmax = (float)(cam.resolution[0] - 1), v.hmax = (float)(cam.resolution[1] - 1);
  v.W = cam.resolution[0], v.R = rows, v.row0 = row0;
  return v;
}

PT_HD float dot3(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
  return (ax * bx + ay * by) + az * bz;
}
PT_HD int32_t float_bits(float f) {
  int32_t i;
  __builtin_memcpy(&i, &f, sizeof i);
  return i;
}
PT_HD float bits_float(int32_t i) {
  float f;
  __builtin_memcpy(&f, &i, sizeof f);
  return f;
}

// The samples the SUM image holds for pixel i: one number for the tile (a float: the forms as they stood), or that number and the
// pixel's extras (Counted: while the extra plane E of the history round is present) — one float add, made before anything else.
struct Counted {
  float samples;
  const float* E;
};
PT_HD float samples_of(float samples, size_t) { return samples; }
PT_HD float samples_of(const Counted& c, size_t i) {
#pragma clang fp contract(off)
  return c.samples + c.E[i];
}

// What pt_denoise's prepare makes of a pixel's feature sums: hit, normal, position; and the object id (0 on a miss).
struct Surface {
  bool hit;
  float nx, ny, nz, px, py, pz;
  int32_t id;
};
template <typename P4>
PT_HD Surface surface(size_t i, size_t npix, const P4* feat) {
#pragma clang fp contract(off)
  const P4 s0 = feat[i], s1 = feat[npix + i], s2 = feat[2 * npix + i];
  Surface s{s1.w > 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0};
  if (s.hit) {
    s.nx = s0.x / s1.w, s.ny = s0.y / s1.w, s.nz = s0.z / s1.w;
    s.px = s2.x / s1.w, s.py = s2.y / s1.w, s.pz = s2.z / s1.w;
    s.id = float_bits(s2.w);
  }
  return s;
}

// The blend of one component: the SUM over `samples` new samples with the history's h over Th samples.  C absent: h = Th = +0.
PT_HD float blend_component(float S, float samples, float h, float Th) {
#pragma clang fp contract(off)
  const float m = h * Th;
  const float a = S + m;
  const float d = samples + Th;
  return a / d;
}

// The variance the fold's planes give one component of the mean of the new samples (pt_noise.h fold_component's last two lines, on
// the planes it left): Tf = (float)T, Df = (float)(M - 1) * Tf.  ptdn::guided_variance is this and the albedo step.
PT_HD float sample_variance(float prev, float q, float Tf, float Df) {
#pragma clang fp contract(off)
  const float d = q - (prev * prev) / Tf;
  return (d > 0.0f ? d : 0.0f) / Df;
}
// The variance of the blend of one component: vn of the new samples' mean, vh of the history's colour.  C absent: Th = vh = +0.
PT_HD float blend_variance(float vn, float samples, float vh, float Th) {
#pragma clang fp contract(off)
  const float dn = samples + Th;
  const float wn = samples / dn;
  const float wh = Th / dn;
  return (wn * wn) * vn + (wh * wh) * vh;
}
// The moments of the blend: x the mean of the new samples of one component, m2h the history's second moment of it; and the blend's
// sum of squared weights from the history's rh (one value per pixel).  C absent: Th = m2h = rh = +0, which gives {x * x, 1}.
struct MomentWeights {
  float wn, wh;
};
PT_HD MomentWeights moment_weights(float samples, float Th) {
#pragma clang fp contract(off)
  const float dn = samples + Th;
  return MomentWeights{samples / dn, Th / dn};
}
PT_HD float blend_moment(float x, float m2h, const MomentWeights& w) {
#pragma clang fp contract(off)
  return w.wn * (x * x) + w.wh * m2h;
}
PT_HD float blend_weight_sum(float rh, const MomentWeights& w) {
#pragma clang fp contract(off)
  return w.wn * w.wn + (w.wh * w.wh) * rh;
}
// {m2b.xyz, rb} of pixel i from the SUM image and the history's {m2h.xyz, rh} (vh; absent: all +0)
// (samples: the pixel's own, samples_of)
template <typename P4>
PT_HD P4 blend_moments(size_t i, const float* S, float samples, float Th, const P4& vh) {
#pragma clang fp contract(off)
  const MomentWeights w = moment_weights(samples, Th);
  const float x = S[3 * i] / samples, y = S[3 * i + 1] / samples, z = S[3 * i + 2] / samples;
  return P4{blend_moment(x, vh.x, w), blend_moment(y, vh.y, w), blend_moment(z, vh.z, w), blend_weight_sum(vh.w, w)};
}
// What travels beside the history: nothing, a variance (PT_HISTORY_VARIANCE) or moments (PT_HISTORY_MOMENTS)
constexpr int kPlain = 0, kVariance = 1, kMoments = 2;
// What the variance side of a capture reads and writes: the fold's two planes with their divisors, VC (or nullptr: absent) and VK.
template <typename P4>
struct VarCapture {
  const P4* noise;
  float Tf, Df;
  const P4* VC;
  P4* VK;
};
// ... and the moments side: VC (or nullptr: absent) and VK; the new samples' part comes from the SUM image itself.
template <typename P4>
struct MomCapture {
  const P4* VC;
  P4* VK;
};
// ... and of a reprojection: VK beside K0, VC beside C.
template <typename P4>
struct VarReproject {
  const P4* VK;
  P4* VC;
};
// ... and the motion of the objects since the capture (PT_HISTORY_MOTION): kMotionRow floats and one kind byte per geom.
constexpr int kMotionRow = 24;
constexpr uint8_t kStill = 0, kMoved = 1, kCarriesNothing = 2;
struct Motion {
  const float* table;
  const uint8_t* kind;
};

// Pixel i of a tile of npix pixels: rgb_avg[3 i ..] = the blend.  C: the current plane, or nullptr (absent).
// Ns: float, or Counted.
template <typename P4, typename Ns>
PT_HD void blend_pixel(size_t i, const float* S, const Ns& samples, const P4* C, float* rgb_avg) {
  const float ns = samples_of(samples, i);
  const P4 c = C ? C[i] : P4{0.0f, 0.0f, 0.0f, 0.0f};
  rgb_avg[3 * i] = blend_component(S[3 * i], ns, c.x, c.w);
  rgb_avg[3 * i + 1] = blend_component(S[3 * i + 1], ns, c.y, c.w);
  rgb_avg[3 * i + 2] = blend_component(S[3 * i + 2], ns, c.z, c.w);
}

// The variance side of a capture: VK[i] = the variance of the blend K0.xyz; Th = C.w of the pixel (C absent: +0).
template <typename P4>
PT_HD void capture_variance_pixel(size_t i, size_t npix, float samples, float Th, const VarCapture<P4>& var) {
#pragma clang fp contract(off)
  const P4 prev = var.noise[i], q = var.noise[npix + i];
  const P4 vh = var.VC ? var.VC[i] : P4{0.0f, 0.0f, 0.0f, 0.0f};
  var.VK[i] = P4{blend_variance(sample_variance(prev.x, q.x, var.Tf, var.Df), samples, vh.x, Th),
                 blend_variance(sample_variance(prev.y, q.y, var.Tf, var.Df), samples, vh.y, Th),
                 blend_variance(sample_variance(prev.z, q.z, var.Tf, var.Df), samples, vh.z, Th), 0.0f};
}
// The moments side of a capture: VK[i] = {m2b.xyz, rb} of the blend K0.xyz; Th = C.w of the pixel (C absent: +0).
template <typename P4>
PT_HD void capture_moments_pixel(size_t i, const float* S, float samples, float Th, const MomCapture<P4>& mom) {
  const P4 vh = mom.VC ? mom.VC[i] : P4{0.0f, 0.0f, 0.0f, 0.0f};
  mom.VK[i] = blend_moments(i, S, samples, Th, vh);
}
// Pixel i: the kept planes K (kKeptPlanes planes of npix) from the SUM image, the feature sums and the current plane (or nullptr).
// kKind: kVariance / kMoments also write VK[i], from `var` (a VarCapture / MomCapture; read only then).
// Ns: float, or Counted (kPlain and kMoments; the fold's variance knows nothing of the extras).
template <int kKind, typename P4, typename Side, typename Ns>
PT_HD void capture_pixel_of(size_t i, size_t npix, const float* S, const P4* feat, const P4* C, const Ns& tile_samples, P4* K, const Side& var) {
#pragma clang fp contract(off)
  const float samples = samples_of(tile_samples, i);
  const Surface s = surface(i, npix, feat);
  const P4 c = C ? C[i] : P4{0.0f, 0.0f, 0.0f, 0.0f};
  K[i] = P4{blend_component(S[3 * i], samples, c.x, c.w), blend_component(S[3 * i + 1], samples, c.y, c.w),
            blend_component(S[3 * i + 2], samples, c.z, c.w), samples + c.w};
  K[npix + i] = P4{s.px, s.py, s.pz, bits_float(s.id)};
  K[2 * npix + i] = P4{s.nx, s.ny, s.nz, 0.0f};
  if constexpr (kKind == kVariance) capture_variance_pixel(i, npix, samples, c.w, var);
  if constexpr (kKind == kMoments) capture_moments_pixel(i, S, samples, c.w, var);
}
template <typename P4>
PT_HD void capture_pixel(size_t i, size_t npix, const float* S, const P4* feat, const P4* C, float samples, P4* K) {
  capture_pixel_of<kPlain>(i, npix, S, feat, C, samples, K, VarCapture<P4>{});
}

// Tile pixel i = (x, r): the history K as seen through the kept camera, resampled at this pixel's first hit.  reject: one byte per
// geom (num_geoms of them), read unless keep_view_dependent; an id outside 1 .. num_geoms is rejected like a listed geom.  A gather:
// of each tap K1 is read first, then K2, and K0 only when the tap passed.  kVar: VK(q) is read after K0, for a tap that passed only;
// vh receives VC's value for the pixel, all zero wherever the pixel is rejected (it is not touched otherwise).  kKind: kPlain reads no
// VK; kVariance interpolates VK.xyz and writes w = +0; kMoments interpolates all four components (w: the sum of squared weights).
//
// kMotion (PT_HISTORY_MOTION): objects moved between the capture and now.  mo.table holds kMotionRow floats per geom — D, the 3 x 4
// map from a point's current position to where it was at the capture, row-major, then Nm, the 3 x 3 map of its normal, then 3 zeros —
// and mo.kind one byte per geom (motion_table below): 0 still, 1 moved, 2 carries nothing.  One step after the first rejections:
// for kind 1 the pixel's p and n become p' = D (p, 1) and n' = Nm n / |Nm n|, and everything after reads those; an id outside
// 1 .. num_geoms (seen only with keep_view_dependent) counts as still.  <..., false> is the body as it stood.
//
// kFeedback (PT_HISTORY_FEEDBACK, with kMoments only): the filtered colour travels beside the raw chain.  FK(q) = {f.xyz, vf} is read
// after VK(q), for a tap that passed only; all four components are interpolated with the weights of the colour, and *fc receives FC's
// value for the pixel, all zero wherever the pixel is rejected.  The cap touches nothing of it.  C and vh are what <.., false> gives.
//
// kTell (the recolour step of PT_HISTORY_MATERIALS): *passed = true where the pixel was not rejected; not touched otherwise, nor without kTell.
template <int kKind, bool kMotion = false, bool kFeedback = false, bool kTell = false, typename P4>
PT_HD P4 reproject_pixel_of(size_t i, const View& v, const P4* K, const P4* feat, const uint8_t* reject, int32_t num_geoms, const Params& P, const P4* VK,
                            P4& vh, const Motion& mo = Motion{}, [[maybe_unused]] const P4* FK = nullptr, [[maybe_unused]] P4* fc = nullptr,
                            [[maybe_unused]] bool* passed = nullptr) {
#pragma clang fp contract(off)
  static_assert(!kFeedback || kKind == kMoments, "the filtered colour travels beside the moments");
  const size_t npix = (size_t)v.W * v.R;
  const P4 zero{0.0f, 0.0f, 0.0f, 0.0f};
  constexpr bool kVar = kKind != kPlain;
  if constexpr (kVar) vh = zero;
  if constexpr (kFeedback) *fc = zero;
  Surface s = surface(i, npix, feat);
  if (!s.hit) return zero;
  if (!P.keep_view_dependent && (s.id < 1 || s.id > num_geoms || reject[s.id - 1])) return zero;
  if constexpr (kMotion) {
    const uint8_t kind = s.id >= 1 && s.id <= num_geoms ? mo.kind[s.id - 1] : (uint8_t)kStill;
    if (kind == kCarriesNothing) return zero;
    if (kind == kMoved) {
      const float* D = mo.table + (size_t)(s.id - 1) * kMotionRow;
      const float* Nm = D + 12;
      const float qx = ((D[0] * s.px + D[1] * s.py) + D[2] * s.pz) + D[3];
      const float qy = ((D[4] * s.px + D[5] * s.py) + D[6] * s.pz) + D[7];
      const float qz = ((D[8] * s.px + D[9] * s.py) + D[10] * s.pz) + D[11];
      const float mx = dot3(Nm[0], Nm[1], Nm[2], s.nx, s.ny, s.nz);
      const float my = dot3(Nm[3], Nm[4], Nm[5], s.nx, s.ny, s.nz);
      const float mz = dot3(Nm[6], Nm[7], Nm[8], s.nx, s.ny, s.nz);
      const float l = dot3(mx, my, mz, mx, my, mz);
      if (!(l > 0.0f)) return zero;
      const float r = __builtin_sqrtf(l);
      s.px = qx, s.py = qy, s.pz = qz;
      s.nx = mx / r, s.ny = my / r, s.nz = mz / r;
    }
  }
  const float vx = s.px - v.pos[0], vy = s.py - v.pos[1], vz = s.pz - v.pos[2];
  const float dz = dot3(vx, vy, vz, v.view[0], v.view[1], v.view[2]);
  if (!(dz > 0.0f)) return zero;
  const float sx = v.hw - dot3(vx, vy, vz, v.right[0], v.right[1], v.right[2]) / (dz * v.plx);
  const float sy = v.hh - dot3(vx, vy, vz, v.up[0], v.up[1], v.up[2]) / (dz * v.ply);
  const float fx = __builtin_floorf(sx), fy = __builtin_floorf(sy);
  if (!(fx >= -1.0f && fx <= v.wmax && fy >= -1.0f && fy <= v.hmax)) return zero;
  const float ax = sx - fx, ay = sy - fy;
  const int ix = (int)fx, iy = (int)fy - v.row0;  // in range: the comparisons above were made in float
  const float tol = P.plane_tol * dz;
  float accx = 0.0f, accy = 0.0f, accz = 0.0f, tacc = 0.0f, wsum = 0.0f;
  [[maybe_unused]] float vaccx = 0.0f, vaccy = 0.0f, vaccz = 0.0f, vaccw = 0.0f;
  [[maybe_unused]] float faccx = 0.0f, faccy = 0.0f, faccz = 0.0f, faccw = 0.0f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int qr = iy + j;
    if (qr < 0 || qr >= v.R) continue;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int qx = ix + t;
      if (qx < 0 || qx >= v.W) continue;
      const size_t q = (size_t)qr * v.W + qx;
      const P4 k1 = K[npix + q];
      if (float_bits(k1.w) != s.id) continue;
      const P4 k2 = K[2 * npix + q];
      if (P.use_dot && dot3(s.nx, s.ny, s.nz, k2.x, k2.y, k2.z) < P.min_dot) continue;
      if (P.use_plane) {
        const float e = dot3(s.nx, s.ny, s.nz, k1.x - s.px, k1.y - s.py, k1.z - s.pz);
        if ((e < 0.0f ? -e : e) > tol) continue;
      }
      const P4 k0 = K[q];
      if (!(k0.w > 0.0f)) continue;
      const float b = (t ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
      accx = accx + b * k0.x, accy = accy + b * k0.y, accz = accz + b * k0.z;
      tacc = tacc + b * k0.w;
      if constexpr (kVar) {
        const P4 vk = VK[q];
        vaccx = vaccx + b * vk.x, vaccy = vaccy + b * vk.y, vaccz = vaccz + b * vk.z;
        if constexpr (kKind == kMoments) vaccw = vaccw + b * vk.w;
      }
      if constexpr (kFeedback) {
        const P4 fk = FK[q];
        faccx = faccx + b * fk.x, faccy = faccy + b * fk.y, faccz = faccz + b * fk.z, faccw = faccw + b * fk.w;
      }
      wsum = wsum + b;
    }
  }
  if (!(wsum >= kMinWeight)) return zero;
  const float tw = tacc / wsum;
  if constexpr (kKind == kVariance) vh = P4{vaccx / wsum, vaccy / wsum, vaccz / wsum, 0.0f};
  if constexpr (kKind == kMoments) vh = P4{vaccx / wsum, vaccy / wsum, vaccz / wsum, vaccw / wsum};
  if constexpr (kFeedback) *fc = P4{faccx / wsum, faccy / wsum, faccz / wsum, faccw / wsum};
  if constexpr (kTell) *passed = true;
  return P4{accx / wsum, accy / wsum, accz / wsum, tw < P.cap ? tw : P.cap};
}
template <typename P4>
PT_HD P4 reproject_pixel(size_t i, const View& v, const P4* K, const P4* feat, const uint8_t* reject, int32_t num_geoms, const Params& P) {
  P4 unused;
  return reproject_pixel_of<kPlain>(i, v, K, feat, reject, num_geoms, P, static_cast<const P4*>(nullptr), unused);
}

// The whole tile on the host.
inline void capture_host(size_t npix, const float* S, const float* feat, const float* C, float samples, float* K) {
  for (size_t i = 0; i < npix; ++i)
    capture_pixel(i, npix, S, reinterpret_cast<const F4*>(feat), reinterpret_cast<const F4*>(C), samples, reinterpret_cast<F4*>(K));
}
inline void reproject_host(const View& v, const float* K, const float* feat, const uint8_t* reject, int32_t num_geoms, const Params& P, float* C) {
  const size_t npix = (size_t)v.W * v.R;
  F4* out = reinterpret_cast<F4*>(C);
  for (size_t i = 0; i < npix; ++i) out[i] = reproject_pixel(i, v, reinterpret_cast<const F4*>(K), reinterpret_cast<const F4*>(feat), reject, num_geoms, P);
}
// ... and with the variance side: VK beside K's capture (which capture_host makes), C and VC in one pass of the lookup.
inline void capture_variance_host(size_t npix, const float* noise, float Tf, float Df, float samples, const float* C, const float* VC, float* VK) {
  const F4* c4 = reinterpret_cast<const F4*>(C);
  const VarCapture<F4> var{reinterpret_cast<const F4*>(noise), Tf, Df, reinterpret_cast<const F4*>(VC), reinterpret_cast<F4*>(VK)};
  for (size_t i = 0; i < npix; ++i) capture_variance_pixel(i, npix, samples, c4 ? c4[i].w : 0.0f, var);  // (K: capture_host, from the image and the features)
}
// ... and the moments side: VK beside K's capture, C and VC = {m2h.xyz, rh} in one pass of the lookup
inline void capture_moments_host(size_t npix, const float* S, float samples, const float* C, const float* VC, float* VK) {
  const F4* c4 = reinterpret_cast<const F4*>(C);
  const MomCapture<F4> mom{reinterpret_cast<const F4*>(VC), reinterpret_cast<F4*>(VK)};
  for (size_t i = 0; i < npix; ++i) capture_moments_pixel(i, S, samples, c4 ? c4[i].w : 0.0f, mom);
}
template <int kKind>
inline void reproject_with_host(const View& v, const float* K, const float* feat, const uint8_t* reject, int32_t num_geoms, const Params& P, const float* VK,
                                float* C, float* VC) {
  const size_t npix = (size_t)v.W * v.R;
  F4 *out = reinterpret_cast<F4*>(C), *vout = reinterpret_cast<F4*>(VC);
  for (size_t i = 0; i < npix; ++i)
    out[i] = reproject_pixel_of<kKind>(i, v, reinterpret_cast<const F4*>(K), reinterpret_cast<const F4*>(feat), reject, num_geoms, P, reinterpret_cast<const F4*>(VK),
                                      vout[i]);
}
inline void reproject_variance_host(const View& v, const float* K, const float* feat, const uint8_t* reject, int32_t num_geoms, const Params& P, const float* VK,
                                    float* C, float* VC) {
  reproject_with_host<kVariance>(v, K, feat, reject, num_geoms, P, VK, C, VC);
}
inline void reproject_moments_host(const View& v, const float* K, const float* feat, const uint8_t* reject, int32_t num_geoms, const Params& P, const float* VK,
                                   float* C, float* VC) {
  reproject_with_host<kMoments>(v, K, feat, reject, num_geoms, P, VK, C, VC);
}
// ... and with the objects' motion: kKind as above; VK, VC unused (nullptr) for kPlain.
template <int kKind>
inline void reproject_motion_host(const View& v, const float* K, const float* feat, const uint8_t* reject, int32_t num_geoms, const Params& P, const float* VK,
                                  const Motion& mo, float* C, float* VC) {
  const size_t npix = (size_t)v.W * v.R;
  F4 *out = reinterpret_cast<F4*>(C), *vout = reinterpret_cast<F4*>(VC);
  F4 unused;
  for (size_t i = 0; i < npix; ++i)
    out[i] = reproject_pixel_of<kKind, true>(i, v, reinterpret_cast<const F4*>(K), reinterpret_cast<const F4*>(feat), reject, num_geoms, P,
                                             reinterpret_cast<const F4*>(VK), kKind == kPlain ? unused : vout[i], mo);
}
// ... and with the filtered colour (PT_HISTORY_FEEDBACK): the moments lookup, FK beside VK and FC beside VC; mo: the motion table, or
// nullptr (the lookup without PT_HISTORY_MOTION).
inline void reproject_feedback_host(const View& v, const float* K, const float* feat, const uint8_t* reject, int32_t num_geoms, const Params& P, const float* VK,
                                    const float* FK, const Motion* mo, float* C, float* VC, float* FC) {
  const size_t npix = (size_t)v.W * v.R;
  F4 *out = reinterpret_cast<F4*>(C), *vout = reinterpret_cast<F4*>(VC), *fout = reinterpret_cast<F4*>(FC);
  const F4 *k4 = reinterpret_cast<const F4*>(K), *f4 = reinterpret_cast<const F4*>(feat), *vk4 = reinterpret_cast<const F4*>(VK), *fk4 = reinterpret_cast<const F4*>(FK);
  for (size_t i = 0; i < npix; ++i)
    out[i] = mo ? reproject_pixel_of<kMoments, true, true>(i, v, k4, f4, reject, num_geoms, P, vk4, vout[i], *mo, fk4, &fout[i])
                : reproject_pixel_of<kMoments, false, true>(i, v, k4, f4, reject, num_geoms, P, vk4, vout[i], Motion{}, fk4, &fout[i]);
}
// The motion table of pt_amd.h (pt_history_motion_host): row g and kind[g] from the kept and the current geom g.  Every factor is
// widened to double, the products and sums are plain double operations in the order written, the result is rounded to float once.
inline bool same_matrices(const PtGeom& k, const PtGeom& c) {  // the 48 matrix words, bytewise
  return __builtin_memcmp(k.transform, c.transform, 64) == 0 && __builtin_memcmp(k.inverseTransform, c.inverseTransform, 64) == 0 &&
         __builtin_memcmp(k.invTranspose, c.invTranspose, 64) == 0;
}
inline void motion_table(const PtGeom* kept, const PtGeom* cur, int n, float* table, uint8_t* kind) {
#pragma clang fp contract(off)
  for (int g = 0; g < n; ++g) {
    float* row = table + (size_t)g * kMotionRow;
    const PtGeom &k = kept[g], &c = cur[g];
    auto at = [](const float* m, int r, int col) { return (double)m[col * 4 + r]; };  // column-major
    for (int r = 0; r < 3; ++r)
      for (int col = 0; col < 4; ++col)
        row[r * 4 + col] = (float)(((at(k.transform, r, 0) * at(c.inverseTransform, 0, col) + at(k.transform, r, 1) * at(c.inverseTransform, 1, col)) +
                                    at(k.transform, r, 2) * at(c.inverseTransform, 2, col)) +
                                   at(k.transform, r, 3) * at(c.inverseTransform, 3, col));
    for (int r = 0; r < 3; ++r)
      for (int col = 0; col < 3; ++col)
        row[12 + r * 3 + col] = (float)((at(k.invTranspose, r, 0) * at(c.transform, col, 0) + at(k.invTranspose, r, 1) * at(c.transform, col, 1)) +
                                        at(k.invTranspose, r, 2) * at(c.transform, col, 2));
    row[21] = row[22] = row[23] = 0.0f;
    const bool same = same_matrices(k, c);
    bool finite = true;
    for (int j = 0; j < 21; ++j) finite = finite && row[j] - row[j] == 0.0f;
    kind[g] = same ? kStill : (k.type == PT_GEOM_TRIANGLE || c.type == PT_GEOM_TRIANGLE || !finite) ? kCarriesNothing : kMoved;
  }
}

// ── the materials' edits since the capture (PT_HISTORY_MATERIALS) ────────────────────────────────────────────────────────
// kRecolorRow floats and one kind byte per geom (recolor_table below): {r_x, r_y, r_z, +0} and 0 unchanged, 1 recoloured, 2 carries nothing.
constexpr int kRecolorRow = 4;
constexpr uint8_t kUnchanged = 0, kRecolored = 1;  // (2: kCarriesNothing)
struct Recolor {
  const float* table;
  const uint8_t* kind;
};
// The lookup with the recolour step: reproject_pixel_of<kKind, kMotion> as it stands — not a line of it changes — with the pixel's
// geom looked at before (kind 2: rejected, C = VC = 0) and the result scaled after (kind 1): h_j = h_j * r_j, vh_j = (vh_j * r_j) * r_j,
// Th and the moments' rh untouched, for a pixel that was not rejected (kTell: a rejected pixel keeps +0 in every word even where r_j
// is -0).  An id outside 1 .. num_geoms counts as unchanged.  The row is one 16-byte load.
template <int kKind, bool kMotion, typename P4>
PT_HD P4 reproject_pixel_materials(size_t i, const View& v, const P4* K, const P4* feat, const uint8_t* reject, int32_t num_geoms, const Params& P, const P4* VK,
                                   P4& vh, const Motion& mo, const Recolor& rc) {
#pragma clang fp contract(off)
  const size_t npix = (size_t)v.W * v.R;
  const Surface s = surface(i, npix, feat);
  const uint8_t kind = s.hit && s.id >= 1 && s.id <= num_geoms ? rc.kind[s.id - 1] : (uint8_t)kUnchanged;
  if (kind == kCarriesNothing) {
    if constexpr (kKind != kPlain) vh = P4{0.0f, 0.0f, 0.0f, 0.0f};
    return P4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  bool passed = false;
  P4 c = reproject_pixel_of<kKind, kMotion, false, true>(i, v, K, feat, reject, num_geoms, P, VK, vh, mo, static_cast<const P4*>(nullptr), static_cast<P4*>(nullptr), &passed);
  if (kind == kRecolored && passed) {
    const P4 r = reinterpret_cast<const P4*>(rc.table)[s.id - 1];
    c.x = c.x * r.x, c.y = c.y * r.y, c.z = c.z * r.z;
    if constexpr (kKind != kPlain) vh.x = (vh.x * r.x) * r.x, vh.y = (vh.y * r.y) * r.y, vh.z = (vh.z * r.z) * r.z;
  }
  return c;
}
// The whole tile on the host; mo: the motion table, or nullptr (the lookup without PT_HISTORY_MOTION).  VK, VC unused (nullptr) for kPlain.
template <int kKind>
inline void reproject_materials_host(const View& v, const float* K, const float* feat, const uint8_t* reject, int32_t num_geoms, const Params& P, const float* VK,
                                     const Motion* mo, const Recolor& rc, float* C, float* VC) {
  const size_t npix = (size_t)v.W * v.R;
  F4 *out = reinterpret_cast<F4*>(C), *vout = reinterpret_cast<F4*>(VC);
  const F4 *k4 = reinterpret_cast<const F4*>(K), *f4 = reinterpret_cast<const F4*>(feat), *vk4 = reinterpret_cast<const F4*>(VK);
  F4 unused;
  for (size_t i = 0; i < npix; ++i)
    out[i] = mo ? reproject_pixel_materials<kKind, true>(i, v, k4, f4, reject, num_geoms, P, vk4, kKind == kPlain ? unused : vout[i], *mo, rc)
                : reproject_pixel_materials<kKind, false>(i, v, k4, f4, reject, num_geoms, P, vk4, kKind == kPlain ? unused : vout[i], Motion{}, rc);
}
// The recolour table of pt_amd.h (pt_history_recolor_host): mk per material from the kept and the current one, then row g and kind[g]
// from geoms[g].materialid (a material id outside 0 .. num_materials - 1: unchanged).  mk and ratio: num_materials entries of scratch.
inline uint8_t recolor_material(const PtMaterial& k, const PtMaterial& c, float ratio[3]) {
#pragma clang fp contract(off)
  ratio[0] = ratio[1] = ratio[2] = 0.0f;
  const bool rest_same = __builtin_memcmp(k.specular_color, c.specular_color, 12) == 0 && __builtin_memcmp(&k.hasReflective, &c.hasReflective, 4) == 0 &&
                         __builtin_memcmp(&k.hasRefractive, &c.hasRefractive, 4) == 0 && __builtin_memcmp(&k.emittance, &c.emittance, 4) == 0;
  if (rest_same && __builtin_memcmp(k.color, c.color, 12) == 0) return kUnchanged;
  if (!rest_same || k.emittance > 0.0f || k.hasReflective > 0.0f) return kCarriesNothing;
  float r[3];
  for (int j = 0; j < 3; ++j) {
    if (!(k.color[j] > 0.0f) || !(c.color[j] >= 0.0f)) return kCarriesNothing;
    r[j] = c.color[j] / k.color[j];
    if (!(r[j] - r[j] == 0.0f)) return kCarriesNothing;
  }
  ratio[0] = r[0], ratio[1] = r[1], ratio[2] = r[2];
  return kRecolored;
}
inline void recolor_table(const PtMaterial* kept, const PtMaterial* cur, int num_materials, const PtGeom* geoms, int num_geoms, float* table, uint8_t* kind) {
  for (int g = 0; g < num_geoms; ++g) {
    float* row = table + (size_t)g * kRecolorRow;
    row[0] = row[1] = row[2] = row[3] = 0.0f;
    const int32_t m = geoms[g].materialid;
    kind[g] = m >= 0 && m < num_materials ? recolor_material(kept[m], cur[m], row) : kUnchanged;
  }
}
inline void blend_host(size_t npix, const float* S, float samples, const float* C, float* rgb_avg) {
  for (size_t i = 0; i < npix; ++i) blend_pixel(i, S, samples, reinterpret_cast<const F4*>(C), rgb_avg);
}

// ── the noise estimate of the blend (pt_history_noise) ───────────────────────────────────────────────────────────────────
// w of one pixel: the blend's variance vb summed over the channels, from the two words the fold left for the pixel (prev, q: any
// float4 type), Tf and Df of the folds so far, and the pixel's Th = C.w and vh = VC (C absent: Th = +0, vh all +0).  With C absent
// wn = 1 and wh = +0, so w is the fold's own plane-0 .w bit for bit.
template <typename N4, typename P4>
PT_HD float noise_value(const N4& prev, const N4& q, float Tf, float Df, float samples, float Th, const P4& vh) {
#pragma clang fp contract(off)
  const float vx = blend_variance(sample_variance(prev.x, q.x, Tf, Df), samples, vh.x, Th);
  const float vy = blend_variance(sample_variance(prev.y, q.y, Tf, Df), samples, vh.y, Th);
  const float vz = blend_variance(sample_variance(prev.z, q.z, Tf, Df), samples, vh.z, Th);
  return (vx + vy) + vz;
}
// Pixel i of a tile of npix pixels: noise = the fold's two planes; C, VC the current plane and its variance, or both nullptr.
template <typename N4, typename P4>
PT_HD float noise_pixel(size_t i, size_t npix, const N4* noise, float Tf, float Df, float samples, const P4* C, const P4* VC) {
  const P4 zero{0.0f, 0.0f, 0.0f, 0.0f};
  return noise_value(noise[i], noise[npix + i], Tf, Df, samples, C ? C[i].w : 0.0f, VC ? VC[i] : zero);
}
// The whole tile on the host; W (or nullptr) receives the plane, the estimates are added in pixel order.
inline double noise_host(size_t npix, const float* noise, float Tf, float Df, float samples, const float* C, const float* VC, float* W) {
  double sse = 0.0;
  for (size_t i = 0; i < npix; ++i) {
    const float w = noise_pixel(i, npix, reinterpret_cast<const F4*>(noise), Tf, Df, samples, reinterpret_cast<const F4*>(C), reinterpret_cast<const F4*>(VC));
    if (W) W[i] = w;
    sse += (double)w;
  }
  return sse;
}

// ── threshold rounds over the blend (pt_history_round_threshold; the kernels: pt_history_threshold.hip) ─────────────────────────
// The steps above with the sample counts of every pixel, cnt = {T_p, M_p}: Tf = (float)T_p, Df = (float)(M_p - 1) * Tf.  Counts names
// them for pixel i: the plane `cnt` of the adaptive state, or (cnt == nullptr, the uniform state) the fold's T and M for every pixel.
struct Counts {
  const ptad::Cnt* cnt;
  int32_t T, M;
};
struct Divisors {
  float Tf, Df;
};
PT_HD Divisors divisors_of(const Counts& c, size_t i) {
#pragma clang fp contract(off)
  const int32_t T = c.cnt ? c.cnt[i].T : c.T, M = c.cnt ? c.cnt[i].M : c.M;
  const float Tf = (float)T;
  return Divisors{Tf, (float)(M - 1) * Tf};
}
// {vb.xyz, +0} of pixel i: the variance of the blend per channel (pass A; what the capture keeps as VK).  noise: the fold's two
// planes (N4: any float4 type); Th = C.w of the pixel and vh = VC (C absent: Th = +0, vh all +0).
template <typename N4, typename P4>
PT_HD P4 blend_variance_pixel(size_t i, size_t npix, const N4* noise, const Divisors& d, float Th, const P4& vh) {
  const N4 prev = noise[i], q = noise[npix + i];
  return P4{blend_variance(sample_variance(prev.x, q.x, d.Tf, d.Df), d.Tf, vh.x, Th), blend_variance(sample_variance(prev.y, q.y, d.Tf, d.Df), d.Tf, vh.y, Th),
            blend_variance(sample_variance(prev.z, q.z, d.Tf, d.Df), d.Tf, vh.z, Th), 0.0f};
}
// Pass A for pixel i: W[i] = (vb.x + vb.y) + vb.z, NE[i] = Tf + Th, the blend's effective sample count.  C, VC: both or nullptr.
// vb (or nullptr): receives {vb.xyz, +0}.  Returns W[i].
template <typename N4, typename P4>
PT_HD float noise_counts_pixel(size_t i, size_t npix, const N4* noise, const Counts& cnt, const P4* C, const P4* VC, float* W, float* NE, P4* vb) {
#pragma clang fp contract(off)
  const Divisors d = divisors_of(cnt, i);
  const float Th = C ? C[i].w : 0.0f;
  const P4 v = blend_variance_pixel(i, npix, noise, d, Th, VC ? VC[i] : P4{0.0f, 0.0f, 0.0f, 0.0f});
  const float w = (v.x + v.y) + v.z;
  W[i] = w;
  NE[i] = d.Tf + Th;
  if (vb) vb[i] = v;
  return w;
}
// Pass B for pixel (x, y) of a tile of W x R: ptad::key_pixel's arithmetic over (Wp, NE) in place of (plane0.w, T) — the 3 x 3
// binomial prefilter of the per-sample variance s = Wp * NE, back in the unit of Wp.
PT_HD uint32_t key_blend_pixel(int x, int y, int W, int R, const float* Wp, const float* NE) {
#pragma clang fp contract(off)
  float num = 0.0f, den = 0.0f;
  for (int j = -1; j <= 1; ++j) {
    const int yy = y + j;
    if (yy < 0 || yy >= R) continue;
    for (int i = -1; i <= 1; ++i) {
      const int xx = x + i;
      if (xx < 0 || xx >= W) continue;
      const size_t q = (size_t)yy * W + xx;
      const float g = (j == 0 ? 0.5f : 0.25f) * (i == 0 ? 0.5f : 0.25f);
      const float s = Wp[q] * NE[q];
      num = num + g * s;
      den = den + g;
    }
  }
  const float f = num / den;
  return ptad::key_bits(f / NE[(size_t)y * W + x]);
}
// The blend of pixel i with the pixel's own count: blend_pixel with samples = Tf_p.
template <typename P4>
PT_HD void blend_counts_pixel(size_t i, const float* S, const Counts& cnt, const P4* C, float* rgb_avg) {
  blend_pixel(i, S, divisors_of(cnt, i).Tf, C, rgb_avg);
}
// The capture of pixel i with the pixel's own counts: capture_pixel_of<kVariance> with samples = Tf_p and the pixel's divisors, so
// K0 = {blend, Tf_p + Th}, K1 and K2 the capture's, VK = {vb.xyz, +0} of pass A.
template <typename P4, typename N4>
PT_HD void capture_counts_pixel(size_t i, size_t npix, const float* S, const P4* feat, const N4* noise, const Counts& cnt, const P4* C, const P4* VC, P4* K,
                                P4* VK) {
  const Divisors d = divisors_of(cnt, i);
  capture_pixel_of<kPlain>(i, npix, S, feat, C, d.Tf, K, VarCapture<P4>{});
  VK[i] = blend_variance_pixel(i, npix, noise, d, C ? C[i].w : 0.0f, VC ? VC[i] : P4{0.0f, 0.0f, 0.0f, 0.0f});
}

// The whole tile on the host.  counts: npix * {T_p, M_p}.  W, NE: npix floats; vb (or nullptr): npix float4.  The estimates are added
// in pixel order.
inline double noise_counts_host(size_t npix, const float* noise, const int32_t* counts, const float* C, const float* VC, float* W, float* NE, float* vb) {
  const Counts cnt{reinterpret_cast<const ptad::Cnt*>(counts), 0, 0};
  double sse = 0.0;
  for (size_t i = 0; i < npix; ++i)
    sse += (double)noise_counts_pixel(i, npix, reinterpret_cast<const F4*>(noise), cnt, reinterpret_cast<const F4*>(C), reinterpret_cast<const F4*>(VC), W, NE,
                                      reinterpret_cast<F4*>(vb));
  return sse;
}
inline std::vector<uint32_t> keys_blend_host(int W, int R, const float* Wp, const float* NE) {
  std::vector<uint32_t> key((size_t)W * R);
  for (int y = 0; y < R; ++y)
    for (int x = 0; x < W; ++x) key[(size_t)y * W + x] = key_blend_pixel(x, y, W, R, Wp, NE);
  return key;
}
// The selection by threshold on the blend's keys: passes A and B, then ptad::select_threshold_host's steps on those keys.
inline void select_threshold_blend_host(int W, int R, const float* noise, const int32_t* counts, const float* C, const float* VC, float threshold, int cap,
                                        int32_t* list, int* above, int* m) {
  const size_t npix = (size_t)W * R;
  std::vector<float> Wp(npix), NE(npix);
  noise_counts_host(npix, noise, counts, C, VC, Wp.data(), NE.data(), nullptr);
  const std::vector<uint32_t> key = keys_blend_host(W, R, Wp.data(), NE.data());
  const uint32_t thr = ptad::threshold_bits(threshold);
  const ptad::Cut top = ptad::cut_host(key, cap);
  uint32_t n_above = 0;
  for (uint32_t k : key) n_above += ptad::above_threshold(k, thr) ? 1u : 0u;
  ptad::scatter_host(key, ptad::threshold_cut(top.tau, top.r, thr), list);
  *above = (int)n_above;
  *m = (int)ptad::threshold_length(n_above, (uint32_t)cap);
}
inline void blend_counts_host(size_t npix, const float* S, const int32_t* counts, const float* C, float* rgb_avg) {
  const Counts cnt{reinterpret_cast<const ptad::Cnt*>(counts), 0, 0};
  for (size_t i = 0; i < npix; ++i) blend_counts_pixel(i, S, cnt, reinterpret_cast<const F4*>(C), rgb_avg);
}
inline void capture_counts_host(size_t npix, const float* S, const float* feat, const float* noise, const int32_t* counts, const float* C, const float* VC, float* K,
                                float* VK) {
  const Counts cnt{reinterpret_cast<const ptad::Cnt*>(counts), 0, 0};
  for (size_t i = 0; i < npix; ++i)
    capture_counts_pixel(i, npix, S, reinterpret_cast<const F4*>(feat), reinterpret_cast<const F4*>(noise), cnt, reinterpret_cast<const F4*>(C),
                         reinterpret_cast<const F4*>(VC), reinterpret_cast<F4*>(K), reinterpret_cast<F4*>(VK));
}

// ── the history round (pt_history_round) ─────────────────────────────────────────────────────────────────────────────────
// PtHistoryRoundOptions with the defaults filled in; the message of a refusal, or nullptr.
struct RoundParams {
  float min_history, max_fraction;
};
inline const char* resolve_round(const PtHistoryRoundOptions* opt, RoundParams* out) {
  PtHistoryRoundOptions o{};
  if (opt) o = *opt;
  if (!(o.min_history - o.min_history == 0.0f) || !(o.max_fraction - o.max_fraction == 0.0f)) return "an option is not finite";
  if (o.min_history == 0.0f) o.min_history = PT_HISTORY_ROUND_MIN_HISTORY;
  if (!(o.min_history > 0.0f)) return "min_history must be positive";
  if (o.max_fraction == 0.0f) o.max_fraction = 1.0f;
  if (!(o.max_fraction > 0.0f && o.max_fraction <= 1.0f)) return "max_fraction is not in (0, 1]";
  *out = RoundParams{o.min_history, o.max_fraction};
  return nullptr;
}
// The key of tile pixel i as its uint32 bit pattern: how far the carried weight Th = C.w lies below min_history, +0 for a miss, an id
// outside 1 .. num_geoms or an emitter (emitter: one byte per geom), and for a history that is long enough.  C == nullptr: absent,
// Th = +0.  Of the feature sums only s1.w and s2.w are read, of C only its w.  A pixel is FRESH when the bits are > 0; a NaN Th gives
// d > 0 false and so +0.
template <typename P4>
PT_HD uint32_t round_key(size_t i, size_t npix, const P4* feat, const P4* C, const uint8_t* emitter, int32_t num_geoms, float min_history) {
#pragma clang fp contract(off)
  const float hitw = feat[npix + i].w;
  const int32_t id = float_bits(feat[2 * npix + i].w);
  if (!(hitw > 0.0f) || id < 1 || id > num_geoms || emitter[id - 1]) return 0u;
  const float Th = C ? C[i].w : 0.0f;
  const float d = min_history - Th;
  return d > 0.0f ? (uint32_t)float_bits(d) : 0u;
}
// List entry i of the merge: the worker's group sum Sw[i] of G iterations joins tile pixel p = list[i], and E_p counts them (gf = (float)G).
PT_HD void merge_entry(size_t i, const int32_t* list, const float* Sw, float gf, float* S, float* E) {
#pragma clang fp contract(off)
  const size_t p = (size_t)list[i];
  S[3 * p] = S[3 * p] + Sw[3 * i];
  S[3 * p + 1] = S[3 * p + 1] + Sw[3 * i + 1];
  S[3 * p + 2] = S[3 * p + 2] + Sw[3 * i + 2];
  E[p] = E[p] + gf;
}

inline std::vector<uint32_t> round_keys_host(size_t npix, const float* feat, const float* C, const uint8_t* emitter, int32_t num_geoms, float min_history) {
  std::vector<uint32_t> key(npix);
  for (size_t i = 0; i < npix; ++i)
    key[i] = round_key(i, npix, reinterpret_cast<const F4*>(feat), reinterpret_cast<const F4*>(C), emitter, num_geoms, min_history);
  return key;
}
// The selection on the host: pt_adaptive.h's selection by threshold on these keys with threshold bits 0 — the cut for rank cap, the
// clamp under the threshold, the scatter.  list holds cap entries; those behind *m keep what they held.
inline void select_host(size_t npix, const float* feat, const float* C, const uint8_t* emitter, int32_t num_geoms, float min_history, int cap, int32_t* list,
                        int* fresh, int* m) {
  const std::vector<uint32_t> key = round_keys_host(npix, feat, C, emitter, num_geoms, min_history);
  const ptad::Cut top = ptad::cut_host(key, cap);
  uint32_t n_fresh = 0;
  for (uint32_t k : key) n_fresh += ptad::above_threshold(k, 0u) ? 1u : 0u;
  ptad::scatter_host(key, ptad::threshold_cut(top.tau, top.r, 0u), list);
  *fresh = (int)n_fresh;
  *m = (int)ptad::threshold_length(n_fresh, (uint32_t)cap);
}
inline void merge_host(float* S, float* E, const int32_t* list, int m, const float* Sw, int group_iters) {
  for (int i = 0; i < m; ++i) merge_entry((size_t)i, list, Sw, (float)group_iters, S, E);
}
// The counted forms of the whole-tile loops above: E_p extras beside the tile's `samples`.
inline void blend_counted_host(size_t npix, const float* S, float samples, const float* E, const float* C, float* rgb_avg) {
  for (size_t i = 0; i < npix; ++i) blend_pixel(i, S, Counted{samples, E}, reinterpret_cast<const F4*>(C), rgb_avg);
}
inline void capture_counted_host(size_t npix, const float* S, const float* feat, const float* C, float samples, const float* E, float* K) {
  for (size_t i = 0; i < npix; ++i)
    capture_pixel_of<kPlain>(i, npix, S, reinterpret_cast<const F4*>(feat), reinterpret_cast<const F4*>(C), Counted{samples, E}, reinterpret_cast<F4*>(K),
                             VarCapture<F4>{});
}
inline void capture_moments_counted_host(size_t npix, const float* S, float samples, const float* E, const float* C, const float* VC, float* VK) {
  const F4* c4 = reinterpret_cast<const F4*>(C);
  const MomCapture<F4> mom{reinterpret_cast<const F4*>(VC), reinterpret_cast<F4*>(VK)};
  for (size_t i = 0; i < npix; ++i) capture_moments_pixel(i, S, samples_of(Counted{samples, E}, i), c4 ? c4[i].w : 0.0f, mom);
}

// ── the history probes (pt_history_probe_keep / _check) ──────────────────────────────────────────────────────────────────
// A sparse grid of last view's samples, rendered again in the world as it is now: a sample is a pure function of (iteration, pixel,
// world), so the two sums differ exactly where a path met something that changed.  What the difference finds is written into C.w,
// the carried weight, which everything downstream reads already.  probe_grid places the probes, probe_keep is what is kept of one,
// probe_gradient compares a kept probe with its replay, probe_apply shortens the history of one tile pixel.
struct ProbeGrid {
  int ox, oy, PW, PR;  // probe (i, j) sits at tile pixel (3 i + ox, 3 j + oy); i < PW, j < PR
};
PT_HD ProbeGrid probe_grid(int W, int R, int phase) {
  const int ox = phase % 3, oy = phase / 3;
  return ProbeGrid{ox, oy, W > ox ? (W - ox + 2) / 3 : 0, R > oy ? (R - oy + 2) / 3 : 0};
}
PT_HD int probe_count(const ProbeGrid& pg) { return pg.PW * pg.PR; }
// the tile pixel of probe s = j * PW + i: ascending in s
PT_HD int32_t probe_pixel(const ProbeGrid& pg, int W, int s) { return (3 * (s / pg.PW) + pg.oy) * W + 3 * (s % pg.PW) + pg.ox; }
// PtHistoryProbeOptions with the defaults filled in; the message of a refusal, or nullptr.
struct ProbeParams {
  int radius;
  float gain;
};
inline const char* resolve_probe(const PtHistoryProbeOptions* opt, ProbeParams* out) {
  PtHistoryProbeOptions o{};
  if (opt) o = *opt;
  if (o.radius == 0) o.radius = PT_HISTORY_PROBE_RADIUS;
  if (o.radius == -1) o.radius = 0;
  if (o.radius < 0 || o.radius > 4) return "radius is 1 .. 4, or -1 for 0";
  if (!(o.gain - o.gain == 0.0f)) return "an option is not finite";
  if (o.gain == 0.0f) o.gain = PT_HISTORY_PROBE_GAIN;
  if (!(o.gain > 0.0f)) return "gain must be positive";
  *out = ProbeParams{o.radius, o.gain};
  return nullptr;
}
// What is kept of the probe at tile pixel p: its sum and the id of its first hit (0 on a miss), read as the capture reads it.
template <typename P4>
PT_HD P4 probe_keep(size_t p, size_t npix, const float* S, const P4* feat) {
  const int32_t id = feat[npix + p].w > 0.0f ? float_bits(feat[2 * npix + p].w) : 0;
  return P4{S[3 * p], S[3 * p + 1], S[3 * p + 2], bits_float(id)};
}
// L[s] of the kept probe k at tile pixel p against its replay Sw[3 s ..]: -1 skipped (the pixel shows another object now, nothing, an
// id outside 1 .. num_geoms or a geom that moved: moved, one byte per geom), else the relative difference of the two sums, at most 1;
// a NaN reads as 1.  Exactly +0 where the replayed paths met nothing that changed.
template <typename P4>
PT_HD float probe_gradient(size_t s, size_t p, size_t npix, const P4& k, const float* Sw, const P4* feat, const uint8_t* moved, int32_t num_geoms) {
#pragma clang fp contract(off)
  const int32_t id = feat[npix + p].w > 0.0f ? float_bits(feat[2 * npix + p].w) : 0;
  if (id != float_bits(k.w) || id < 1 || id > num_geoms || moved[id - 1]) return -1.0f;
  const float wx = Sw[3 * s], wy = Sw[3 * s + 1], wz = Sw[3 * s + 2];
  const float d = (__builtin_fabsf(wx - k.x) + __builtin_fabsf(wy - k.y)) + __builtin_fabsf(wz - k.z);
  const float mo = (k.x + k.y) + k.z, mw = (wx + wy) + wz;
  const float m = mo > mw ? mo : mw;
  const float lam = m > 0.0f ? d / m : 0.0f;
  return lam < 1.0f ? lam : 1.0f;
}
// Tile pixel i = (x, r): C.w shortened by the largest L of the probes within `radius` probe cells; every word kept for a miss, an id
// outside 1 .. num_geoms, a moved geom (PT_HISTORY_MOTION's business) and where that maximum is 0.  Only C[i].w is read and written.
template <typename P4>
PT_HD void probe_apply(size_t i, int W, int R, const ProbeGrid& pg, const float* L, const P4* feat, const uint8_t* moved, int32_t num_geoms,
                       const ProbeParams& P, P4* C) {
#pragma clang fp contract(off)
  const size_t npix = (size_t)W * R;
  const int32_t id = float_bits(feat[2 * npix + i].w);
  if (!(feat[npix + i].w > 0.0f) || id < 1 || id > num_geoms || moved[id - 1]) return;
  const int x = (int)(i % (size_t)W), r = (int)(i / (size_t)W);
  const int i0 = x / 3, j0 = r / 3;
  float lam = 0.0f;
  for (int j = j0 - P.radius; j <= j0 + P.radius; ++j) {
    if (j < 0 || j >= pg.PR) continue;
    for (int ii = i0 - P.radius; ii <= i0 + P.radius; ++ii) {
      if (ii < 0 || ii >= pg.PW) continue;
      const float l = L[(size_t)j * pg.PW + ii];
      lam = l > lam ? l : lam;
    }
  }
  if (!(lam > 0.0f)) return;
  float g = lam * P.gain;
  g = g < 1.0f ? g : 1.0f;
  C[i].w = C[i].w * (1.0f - g);
}
// 1 where the 48 matrix words of geom g differ bytewise from the kept geom's: motion_table's kind != kStill
inline void probe_moved(const PtGeom* kept, const PtGeom* cur, int n, uint8_t* moved) {
  for (int g = 0; g < n; ++g) moved[g] = same_matrices(kept[g], cur[g]) ? 0 : 1;
}
// The whole tile on the host.
inline void probe_keep_host(int W, int R, int phase, const float* S, const float* feat, float* kept) {
  const ProbeGrid pg = probe_grid(W, R, phase);
  for (int s = 0; s < probe_count(pg); ++s)
    reinterpret_cast<F4*>(kept)[s] = probe_keep((size_t)probe_pixel(pg, W, s), (size_t)W * R, S, reinterpret_cast<const F4*>(feat));
}
inline void probe_gradient_host(int W, int R, int phase, const float* kept, const float* Sw, const float* feat, const uint8_t* moved, int32_t num_geoms,
                                float* L, int* changed, int* skipped) {
  const ProbeGrid pg = probe_grid(W, R, phase);
  int nc = 0, ns = 0;
  for (int s = 0; s < probe_count(pg); ++s) {
    L[s] = probe_gradient((size_t)s, (size_t)probe_pixel(pg, W, s), (size_t)W * R, reinterpret_cast<const F4*>(kept)[s], Sw, reinterpret_cast<const F4*>(feat),
                          moved, num_geoms);
    nc += L[s] > 0.0f, ns += L[s] < 0.0f;
  }
  if (changed) *changed = nc;
  if (skipped) *skipped = ns;
}
inline void probe_apply_host(int W, int R, int phase, const float* L, const float* feat, const uint8_t* moved, int32_t num_geoms, const ProbeParams& P, float* C) {
  const ProbeGrid pg = probe_grid(W, R, phase);
  for (size_t i = 0; i < (size_t)W * R; ++i) probe_apply(i, W, R, pg, L, reinterpret_cast<const F4*>(feat), moved, num_geoms, P, reinterpret_cast<F4*>(C));
}

}  // namespace pthi
