// The host side of the feedback, stand-alone: pt_history.h and pt_denoise.h are plain C++, so the system compiler builds this with
// -fsanitize=address,undefined and tests/test_history_feedback_host.py runs it directly.
// The loops of that test, once: the three tiles (37 x 23 at rows 5 .. 27 of a 37 x 33 frame, 64 x 4, 5 x 1), the filter's levels 1 .. 3,
// the tap after the first and after the last level, both variance rules, the extra plane absent and present, the motion table absent and
// present.  Per case three views of a made-up wall at 1 spp: the lookup with the filtered colour, the feedback filter with its tap, the
// capture, and the tap promoted to FK.  Every array is exactly as large as the functions may touch, on the heap, so an access past an
// end is reported; the exit status is 0 and one line is printed when nothing was.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pt_denoise.h"
#include "pt_history.h"

static uint32_t g_state = 13579u;
static float rnd() {  // [0, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

struct Tile {
  int W, R, row0, H;
};

// One case; the sum of the last view's filtered image and tap, or a negative value: something was left unwritten or marked.
static double run(const Tile& t, int levels, int level, int variance, bool extras, bool motion) {
  const int W = t.W, R = t.R;
  const size_t n = (size_t)W * R;
  const float samples = 1.0f;
  PtCamera cam{};
  cam.resolution[0] = W, cam.resolution[1] = t.H;
  cam.position[0] = 0.25f, cam.position[1] = 0.5f, cam.position[2] = -6.0f;
  cam.view[2] = 1.0f, cam.up[1] = 1.0f, cam.right[0] = -1.0f;
  cam.pixelLength[0] = cam.pixelLength[1] = 0.03125f;

  // the first hits: a wall at depth 8; the later views' pixels land between the first view's (and past its edges)
  std::vector<float> feat0(12 * n), feat1(12 * n);
  const float depth = 8.0f;
  for (int y = 0; y < R; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t i = (size_t)y * W + x;
      for (int view = 0; view < 2; ++view) {
        std::vector<float>& f = view ? feat1 : feat0;
        const float sx = (float)x + 0.5f + (view ? 1.25f : 0.0f), sy = (float)(y + t.row0) + 0.5f + (view ? -0.75f : 0.0f);
        const float px = cam.position[0] - ((float)W * 0.5f - sx) * depth * cam.pixelLength[0];
        const float py = cam.position[1] + ((float)t.H * 0.5f - sy) * depth * cam.pixelLength[1];
        f[4 * i + 2] = -1.0f;                                                                    // normal (0, 0, -1)
        f[4 * (n + i)] = f[4 * (n + i) + 1] = f[4 * (n + i) + 2] = 0.5f, f[4 * (n + i) + 3] = 1.0f;  // albedo | hits
        f[4 * (2 * n + i)] = px, f[4 * (2 * n + i) + 1] = py, f[4 * (2 * n + i) + 2] = cam.position[2] + depth;
        f[4 * (2 * n + i) + 3] = pthi::bits_float(1 + (int32_t)(2 * x >= W));                    // two objects side by side
      }
    }
  if (n > 4) feat1[4 * (n + 3) + 3] = 0.0f;  // a miss

  // the motion table: geom 1 still, geom 2 moved by the identity map written out (kind 1: the arithmetic runs, the place is the same)
  std::vector<float> table(2 * pthi::kMotionRow, 0.0f);
  std::vector<uint8_t> kind = {pthi::kStill, pthi::kMoved};
  for (int g = 0; g < 2; ++g) {
    float* row = table.data() + g * pthi::kMotionRow;
    row[0] = row[5] = row[10] = 1.0f, row[12] = row[16] = row[20] = 1.0f;
  }
  const pthi::Motion mo{table.data(), kind.data()};

  pthi::Params HP{};
  if (pthi::resolve(nullptr, &HP)) return -3.0;
  const uint8_t reject[2] = {0, 0};
  PtDenoiseOptions opt{};
  opt.levels = levels;
  ptdn::Job j{};
  if (ptdn::resolve(&opt, &j.P, ptdn::kHistorySigmaColor)) return -3.0;
  j.form = ptdn::Form::Feedback;
  j.div.samples = samples;
  j.div.fb_variance = variance;
  j.tap_level = level;

  std::vector<float> S(3 * n), E(n), K(12 * n), VK(4 * n), FK(4 * n), C(4 * n), VC(4 * n), FC(4 * n), K2(12 * n), VK2(4 * n), P(4 * n), out(3 * n), var_raw(n);
  std::vector<uint8_t> mark(n);
  for (int v = 0; v < 3; ++v) {
    const std::vector<float>& feat = v ? feat1 : feat0;
    for (size_t i = 0; i < 3 * n; ++i) S[i] = rnd();  // one sample per pixel
    for (size_t i = 0; i < n; ++i) E[i] = extras && i % 3 == 1 ? 3.0f : 0.0f;
    for (size_t i = 0; i < n && extras; ++i)
      if (E[i] > 0.0f) S[3 * i] += rnd() * 3.0f, S[3 * i + 1] += rnd() * 3.0f, S[3 * i + 2] += rnd() * 3.0f;
    const bool have = v > 0;
    if (have)
      pthi::reproject_feedback_host(pthi::make_view(cam, R, t.row0), K.data(), feat.data(), reject, 2, HP, VK.data(), FK.data(), motion ? &mo : nullptr, C.data(),
                                    VC.data(), FC.data());
    j.f = {W, R, S.data(), feat.data(), nullptr, have ? C.data() : nullptr, have ? VC.data() : nullptr, extras ? E.data() : nullptr, have ? FC.data() : nullptr};
    j.tap = P.data();
    ptdn::denoise_host(j, nullptr, out.data(), var_raw.data(), nullptr, mark.data());
    const float* c = have ? C.data() : nullptr;
    if (extras) {
      pthi::capture_counted_host(n, S.data(), feat.data(), c, samples, E.data(), K2.data());
      pthi::capture_moments_counted_host(n, S.data(), samples, E.data(), c, have ? VC.data() : nullptr, VK2.data());
    } else {
      pthi::capture_host(n, S.data(), feat.data(), c, samples, K2.data());
      pthi::capture_moments_host(n, S.data(), samples, c, have ? VC.data() : nullptr, VK2.data());
    }
    K.swap(K2), VK.swap(VK2), FK.swap(P);  // FK := P
    for (size_t i = 0; i < n; ++i)
      if (var_raw[i] < 0.0f) return -5.0;  // a mark the spatial step left behind
  }
  double sum = 0.0;
  for (size_t i = 0; i < 3 * n; ++i) sum += out[i];
  for (size_t i = 0; i < 4 * n; ++i) sum += FK[i];
  return sum == sum ? sum : -4.0;  // (a NaN: something was read that nobody wrote)
}

int main() {
  const Tile tiles[3] = {{37, 23, 5, 33}, {64, 4, 0, 7}, {5, 1, 0, 4}};
  int cases = 0;
  double total = 0.0;
  for (const Tile& t : tiles)
    for (int levels = 1; levels <= 3; ++levels)
      for (int level : {1, levels}) {  // (levels == 1: the same case twice)
        for (int variance = 0; variance < 2; ++variance)
          for (int extras = 0; extras < 2; ++extras)
            for (int motion = 0; motion < 2; ++motion) {
              const double s = run(t, levels, level, variance, extras != 0, motion != 0);
              if (s < 0.0) {
                std::printf("%d x %d levels %d tap %d rule %d extras %d motion %d: %g\n", t.W, t.R, levels, level, variance, extras, motion, s);
                return 4;
              }
              total += s, ++cases;
            }
      }
  std::printf("feedback: %d cases, sum %.9g\n", cases, total);
  return 0;
}
