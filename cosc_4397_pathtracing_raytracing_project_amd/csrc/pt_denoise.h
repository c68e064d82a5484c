// pt_denoise.h — the edge-avoiding à-trous filter of include/pt_amd.h (pt_denoise), ONE implementation of its arithmetic.
//
// The per-pixel prepare / level / finish bodies below are what the HIP kernels (pt_denoise.hip) and the host loop
// (denoise_host, exported as pt_denoise_host) both run, so the two cannot disagree; tests/denoise_ref.py restates them in numpy.
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
#include <vector>

#include "../../include/pt_amd.h"
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
inline const char* resolve(const PtDenoiseOptions* opt, Params* out) {
#pragma clang fp contract(off)
  PtDenoiseOptions o{};
  if (opt) o = *opt;
  if (o.levels == 0) o.levels = 5;
  if (o.levels < 1 || o.levels > kMaxLevels) return "levels outside 1 .. 8";
  const float sig[3] = {o.sigma_color, o.sigma_normal, o.sigma_position};
  const float def[3] = {4.0f, 0.5f, 1.0f};
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

// ── prepare: pixel i of the frame ────────────────────────────────────────────────────────────────────────────────────────
PT_HD void prepare_pixel(size_t i, size_t npix, const float* S, const V4* planes, float samples, int keep_albedo, V4* n, V4* p, V4* a, V4* c) {
#pragma clang fp contract(off)
  const V4 s0 = planes[i], s1 = planes[npix + i], s2 = planes[2 * npix + i];
  const bool hit = s1.w > 0.0f;
  V4 vn{0.0f, 0.0f, 0.0f, hit ? 1.0f : 0.0f}, va{0.0f, 0.0f, 0.0f, 0.0f}, vp{0.0f, 0.0f, 0.0f, 0.0f};
  if (hit) {
    vn.x = s0.x / s1.w, vn.y = s0.y / s1.w, vn.z = s0.z / s1.w;
    va.x = s1.x / s1.w, va.y = s1.y / s1.w, va.z = s1.z / s1.w;
    vp.x = s2.x / s1.w, vp.y = s2.y / s1.w, vp.z = s2.z / s1.w;
  }
  V4 vc{S[3 * i] / samples, S[3 * i + 1] / samples, S[3 * i + 2] / samples, 0.0f};
  if (!keep_albedo) {
    vc.x = va.x > 0.0f ? vc.x / va.x : vc.x;
    vc.y = va.y > 0.0f ? vc.y / va.y : vc.y;
    vc.z = va.z > 0.0f ? vc.z / va.z : vc.z;
  }
  n[i] = vn, p[i] = vp, a[i] = va, c[i] = vc;
}

// ── level: one tap against one centre ────────────────────────────────────────────────────────────────────────────────────
struct Centre {
  V4 c, n, p;  // n.w: the hit flag (1 / 0), or -1: no such pixel (no tap matches it)
  float ax, ay, az, wsum;
};
PT_HD float dist2(const V4& q, const V4& o) {
#pragma clang fp contract(off)
  const float dx = q.x - o.x, dy = q.y - o.y, dz = q.z - o.z;
  return (dx * dx + dy * dy) + dz * dz;
}
PT_HD void tap(Centre& ce, float h, float cf, const Params& P, const V4& qc, const V4& qn, const V4& qp) {
#pragma clang fp contract(off)
  if (qn.w != ce.n.w) return;
  const float dc = dist2(qc, ce.c), dn = dist2(qn, ce.n), dp = dist2(qp, ce.p);
  const float e = (dc * cf + dn * P.inv_n) + dp * P.inv_p;
  const float w = h * ptmath::exp32(-e);
  ce.ax = ce.ax + w * qc.x;
  ce.ay = ce.ay + w * qc.y;
  ce.az = ce.az + w * qc.z;
  ce.wsum = ce.wsum + w;
}

// Threads of a level over a frame of R rows: column x, row slot ty < level_slots(R, l); slot ty filters the rows
// first_row(ty, l) + k * s, k < kRows, that exist.  (Groups of kRows * s rows, one slot per residue of the step.)
PT_HD int level_slots(int R, int l) {
  const int span = kRows << l;
  return ((R + span - 1) / span) << l;
}
PT_HD int first_row(int ty, int l) { return (ty >> l) * (kRows << l) + (ty & ((1 << l) - 1)); }

// Level l for the pixels of column x in slot ty: reads c, n, p, writes `out` (the other colour buffer).
PT_HD void level_column(int W, int R, int x, int ty, int l, const Params& P, const V4* c, const V4* n, const V4* p, V4* out) {
#pragma clang fp contract(off)
  constexpr float H[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
  const int s = 1 << l;
  const int y0 = first_row(ty, l);
  if (y0 >= R) return;  // (a slot of the last, partial group of rows)
  const float cf = color_factor(P, l);
  Centre ce[kRows];
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
        if (j >= -2 && j <= 2) tap(ce[k], H[j + 2] * H[i + 2], cf, P, qc, qn, qp);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int y = y0 + k * s;
    if (y < R) out[(size_t)y * W + x] = V4{ce[k].ax / ce[k].wsum, ce[k].ay / ce[k].wsum, ce[k].az / ce[k].wsum, 0.0f};
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

// The colour buffer that holds c_l (prepare writes c_0 into buffer 0, level l reads l & 1 and writes the other); the finish step
// writes its 12 bytes per pixel over the buffer that does not hold c_levels.
PT_HD int color_buffer(int l) { return l & 1; }

// The whole filter on the host, with the bodies above in the kernels' own thread order.
inline void denoise_host(int W, int R, const float* S, const float* planes, float samples, const Params& P, float* out) {
  const size_t npix = (size_t)W * R;
  std::vector<V4> ws(kWorkspaceV4 * npix);
  V4 *n = ws.data(), *p = n + npix, *a = p + npix, *col[2] = {a + npix, a + 2 * npix};
  std::vector<V4> pl(PT_FEATURE_PLANES * npix);  // (the caller's planes need not be 16-byte aligned)
  for (size_t i = 0; i < pl.size(); ++i) pl[i] = V4{planes[4 * i], planes[4 * i + 1], planes[4 * i + 2], planes[4 * i + 3]};
  for (size_t i = 0; i < npix; ++i) prepare_pixel(i, npix, S, pl.data(), samples, P.keep_albedo, n, p, a, col[0]);
  for (int l = 0; l < P.levels; ++l)
    for (int ty = 0; ty < level_slots(R, l); ++ty)
      for (int x = 0; x < W; ++x) level_column(W, R, x, ty, l, P, col[color_buffer(l)], n, p, col[color_buffer(l + 1)]);
  for (size_t i = 0; i < npix; ++i) finish_pixel(i, P.keep_albedo, col[color_buffer(P.levels)], a, out);
}

}  // namespace ptdn
