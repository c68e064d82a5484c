// The host side of the history's moments and of the filter that reads them, stand-alone: pt_history.h and pt_denoise.h are plain C++,
// so the system compiler builds this with -fsanitize=address,undefined and tests/test_history_moments_host.py runs it directly.
// Five views at 1 spp of a made-up wall at W x R pixels (argv: W R): the first from the kept camera, the others from one a pixel to the
// side.  Per view: the lookup with moments, the filter (prepare, spatial estimate, prefilter, levels, finish), the capture with moments.
// Every array is exactly as large as the functions may touch, on the heap, so an access past an end is reported; the exit status is 0
// and one line is printed when nothing was.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pt_denoise.h"
#include "pt_history.h"

static uint32_t g_state = 24680u;
static float rnd() {  // [0, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int W = std::atoi(argv[1]), R = std::atoi(argv[2]);
  if (W < 1 || R < 1) return 2;
  const size_t n = (size_t)W * R;
  const int views = 5;
  const float samples = 1.0f;

  PtCamera cam{};
  cam.resolution[0] = W, cam.resolution[1] = R;
  cam.position[0] = 0.25f, cam.position[1] = 0.5f, cam.position[2] = -6.0f;
  cam.view[2] = 1.0f, cam.up[1] = 1.0f, cam.right[0] = -1.0f;
  cam.pixelLength[0] = cam.pixelLength[1] = 0.03125f;

  // the first hits: a wall at depth 8; the later views' pixels land between the first view's (and past its edges)
  std::vector<float> feat0(12 * n), feat1(12 * n);
  const float hits = 1.0f, depth = 8.0f;
  for (int y = 0; y < R; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t i = (size_t)y * W + x;
      for (int view = 0; view < 2; ++view) {
        std::vector<float>& f = view ? feat1 : feat0;
        const float sx = (float)x + 0.5f + (view ? 1.25f : 0.0f), sy = (float)y + 0.5f + (view ? -0.75f : 0.0f);
        const float px = cam.position[0] - ((float)W * 0.5f - sx) * depth * cam.pixelLength[0];
        const float py = cam.position[1] + ((float)R * 0.5f - sy) * depth * cam.pixelLength[1];
        f[4 * i + 2] = -1.0f * hits;                                                                              // normal (0, 0, -1) | depth
        f[4 * (n + i)] = f[4 * (n + i) + 1] = f[4 * (n + i) + 2] = 0.5f * hits, f[4 * (n + i) + 3] = hits;      // albedo | hits
        f[4 * (2 * n + i)] = px * hits, f[4 * (2 * n + i) + 1] = py * hits, f[4 * (2 * n + i) + 2] = (cam.position[2] + depth) * hits;
        f[4 * (2 * n + i) + 3] = pthi::bits_float(1 + (int32_t)(2 * y >= R));                                     // two objects, one above the other
      }
    }
  if (n > 4) feat1[4 * (n + 3) + 3] = 0.0f;  // a miss

  pthi::Params HP{};
  if (pthi::resolve(nullptr, &HP)) return 3;
  const uint8_t reject[2] = {0, 0};
  ptdn::Job j{};
  j.form = ptdn::Form::Moments;
  if (ptdn::resolve(nullptr, &j.P, ptdn::kHistorySigmaColor)) return 3;
  j.div.samples = samples;

  std::vector<float> S(3 * n), K(12 * n), VK(4 * n), C(4 * n), VC(4 * n), K2(12 * n), VK2(4 * n), out(3 * n), var_raw(n);
  std::vector<uint8_t> mark(n);
  size_t marked_first = 0, marked_last = 0;
  double sums[3] = {0, 0, 0};
  for (int v = 0; v < views; ++v) {
    const std::vector<float>& feat = v ? feat1 : feat0;
    for (size_t i = 0; i < 3 * n; ++i) S[i] = rnd();  // one sample per pixel
    const bool have = v > 0;
    if (have) pthi::reproject_moments_host(pthi::make_view(cam, R, 0), K.data(), feat.data(), reject, 2, HP, VK.data(), C.data(), VC.data());
    j.f = {W, R, S.data(), feat.data(), nullptr, have ? C.data() : nullptr, have ? VC.data() : nullptr};
    ptdn::denoise_host(j, nullptr, out.data(), var_raw.data(), nullptr, mark.data());
    pthi::capture_host(n, S.data(), feat.data(), have ? C.data() : nullptr, samples, K2.data());
    pthi::capture_moments_host(n, S.data(), samples, have ? C.data() : nullptr, have ? VC.data() : nullptr, VK2.data());
    K.swap(K2), VK.swap(VK2);
    size_t marked = 0;
    for (size_t i = 0; i < n; ++i) {
      marked += mark[i];
      if (var_raw[i] < 0.0f) return 5;  // a mark the spatial step left behind
    }
    if (v == 0) marked_first = marked;
    marked_last = marked;
  }
  for (size_t i = 0; i < n; ++i) {
    sums[0] += VK[4 * i + 3], sums[1] += var_raw[i];
    for (int k = 0; k < 3; ++k) sums[2] += out[3 * i + k];
  }
  std::printf("%d x %d, %d views, marked: %zu first, %zu last, sums r %.9g var_raw %.9g filtered %.9g\n", W, R, views, marked_first, marked_last, sums[0], sums[1],
              sums[2]);
  return sums[2] == sums[2] ? 0 : 4;  // (a NaN in the filtered image: something was read that nobody wrote)
}
