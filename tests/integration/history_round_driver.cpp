// The host side of the history round, stand-alone: pt_history.h and pt_denoise.h are plain C++, so the system compiler builds this with
// -fsanitize=address,undefined and tests/test_history_round_host.py runs it directly.
// Four views at 1 spp of a made-up wall at W x R pixels (argv: W R): the first from the kept camera, the others from one a pixel to the
// side.  Per view: the lookup with moments, the round (key, selection under a cap of a third of the tile, merge of made-up group sums),
// the counted blend, filter and captures.  Every array is exactly as large as the functions may touch, on the heap, so an access past
// an end is reported; the exit status is 0 and one line is printed when nothing was.
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

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int W = std::atoi(argv[1]), R = std::atoi(argv[2]);
  if (W < 1 || R < 1) return 2;
  const size_t n = (size_t)W * R;
  const int views = 4, G = 4;
  const float samples = 1.0f;

  PtCamera cam{};
  cam.resolution[0] = W, cam.resolution[1] = R;
  cam.position[0] = 0.25f, cam.position[1] = 0.5f, cam.position[2] = -6.0f;
  cam.view[2] = 1.0f, cam.up[1] = 1.0f, cam.right[0] = -1.0f;
  cam.pixelLength[0] = cam.pixelLength[1] = 0.03125f;

  // the first hits: a wall at depth 8 of three objects side by side, the third an emitter; the later views' pixels land between the
  // first view's (and past its edges)
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
        f[4 * i + 2] = -1.0f * hits;
        f[4 * (n + i)] = f[4 * (n + i) + 1] = f[4 * (n + i) + 2] = 0.5f * hits, f[4 * (n + i) + 3] = hits;
        f[4 * (2 * n + i)] = px * hits, f[4 * (2 * n + i) + 1] = py * hits, f[4 * (2 * n + i) + 2] = (cam.position[2] + depth) * hits;
        f[4 * (2 * n + i) + 3] = pthi::bits_float(1 + (int32_t)(3 * x / W));
      }
    }
  if (n > 4) feat1[4 * (n + 3) + 3] = 0.0f;                             // a miss
  if (n > 6) feat1[4 * (2 * n + 5) + 3] = pthi::bits_float(4);          // an id past the table
  const uint8_t emitter[3] = {0, 0, 1}, reject[3] = {0, 0, 0};

  pthi::Params HP{};
  pthi::RoundParams RP{};
  PtHistoryRoundOptions ro{};
  ro.max_fraction = 1.0f / 3.0f;
  if (pthi::resolve(nullptr, &HP) || pthi::resolve_round(&ro, &RP)) return 3;
  const int cap = ptad::list_length((double)RP.max_fraction, (int64_t)n);
  ptdn::Job j{};
  j.form = ptdn::Form::Moments;
  if (ptdn::resolve(nullptr, &j.P, ptdn::kHistorySigmaColor)) return 3;
  j.div.samples = samples;

  std::vector<float> S(3 * n), E(n), K(12 * n), VK(4 * n), C(4 * n), VC(4 * n), K2(12 * n), VK2(4 * n), out(3 * n), blend(3 * n);
  std::vector<int32_t> list((size_t)cap);
  size_t selected = 0;
  int fresh_last = 0;
  double sum = 0.0;
  for (int v = 0; v < views; ++v) {
    const std::vector<float>& feat = v ? feat1 : feat0;
    for (size_t i = 0; i < 3 * n; ++i) S[i] = rnd();  // one sample per pixel
    for (size_t i = 0; i < n; ++i) E[i] = 0.0f;       // a new view: the image and its extras start over
    const bool have = v > 0;
    if (have) pthi::reproject_moments_host(pthi::make_view(cam, R, 0), K.data(), feat.data(), reject, 3, HP, VK.data(), C.data(), VC.data());
    int fresh = 0, m = 0;
    pthi::select_host(n, feat.data(), have ? C.data() : nullptr, emitter, 3, RP.min_history, cap, list.data(), &fresh, &m);
    if (m < 0 || m > cap || fresh < m) return 5;
    for (int i = 0; i < m; ++i)
      if (list[(size_t)i] < 0 || (size_t)list[(size_t)i] >= n || (i > 0 && list[(size_t)i] <= list[(size_t)i - 1])) return 6;
    if (m > 0) {
      std::vector<float> Sw(3 * (size_t)m);  // exactly m entries: the merge reads no further
      for (float& x : Sw) x = (float)G * rnd();
      pthi::merge_host(S.data(), E.data(), list.data(), m, Sw.data(), G);
    }
    pthi::blend_counted_host(n, S.data(), samples, E.data(), have ? C.data() : nullptr, blend.data());
    j.f = {W, R, S.data(), feat.data(), nullptr, have ? C.data() : nullptr, have ? VC.data() : nullptr, E.data()};
    ptdn::denoise_host(j, nullptr, out.data());
    pthi::capture_counted_host(n, S.data(), feat.data(), have ? C.data() : nullptr, samples, E.data(), K2.data());
    pthi::capture_moments_counted_host(n, S.data(), samples, E.data(), have ? C.data() : nullptr, have ? VC.data() : nullptr, VK2.data());
    K.swap(K2), VK.swap(VK2);
    selected = (size_t)m, fresh_last = fresh;
  }
  for (size_t i = 0; i < 3 * n; ++i) sum += out[i] + blend[i];
  std::printf("%d x %d, %d views, selected: %zu of %d fresh at the last (cap %d), sum %.9g\n", W, R, views, selected, fresh_last, cap, sum);
  return sum == sum ? 0 : 4;  // (a NaN: something was read that nobody wrote)
}
