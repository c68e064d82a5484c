// The host side of the threshold rounds over the blend, stand-alone: pt_history.h and pt_denoise.h are plain C++, so the system compiler
// builds this with -fsanitize=address,undefined and tests/test_history_threshold_host.py runs it directly.  The shapes of that test
// (97 x 61, 3 x 2, 257 x 5) with made-up planes and counts T_p in 2 .. 40, M_p in 2 .. T_p, the history absent and present: pass A,
// pass B, the selection at three caps, the blend, the capture and the filter.  Every array is exactly as large as the functions may
// touch, on the heap, so an access past an end is reported; the exit status is 0 and one line is printed when nothing was.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pt_denoise.h"
#include "pt_history.h"

static uint32_t g_state = 2463534242u;
static uint32_t rnd_u() {
  g_state = g_state * 1664525u + 1013904223u;
  return g_state >> 8;
}
static float rnd() { return (float)rnd_u() * (1.0f / 16777216.0f); }  // [0, 1)

static int run(int W, int R, bool history, int* cases) {
  const size_t n = (size_t)W * R;
  std::vector<int32_t> counts(2 * n);
  std::vector<float> S(3 * n), noise(4 * PT_NOISE_PLANES * n, 0.0f), feat(4 * PT_FEATURE_PLANES * n, 0.0f), C(4 * n), VC(4 * n);
  for (size_t i = 0; i < n; ++i) {
    const int T = 2 + (int)(rnd_u() % 39), M = 2 + (int)(rnd_u() % (uint32_t)(T - 1));
    counts[2 * i] = T, counts[2 * i + 1] = M;
    const bool gone = i % 4 == 3, hit = i % 6 != 5;
    for (int k = 0; k < 3; ++k) {
      const float s = i % 11 == 10 ? 0.0f : 2.0f * rnd() * (float)T;
      S[3 * i + k] = s;
      noise[4 * i + k] = s;
      noise[4 * (n + i) + k] = (s * s) / (float)T * (i % 5 == 4 ? 1.0f : 1.0f + 0.5f * rnd());
      C[4 * i + k] = gone ? 0.0f : rnd(), VC[4 * i + k] = gone || i % 5 == 0 ? 0.0f : rnd() * 0.01f;
      feat[4 * i + k] = hit ? rnd() : 0.0f, feat[4 * (n + i) + k] = hit ? 0.5f : 0.0f, feat[4 * (2 * n + i) + k] = hit ? 10.0f * rnd() : 0.0f;
    }
    C[4 * i + 3] = gone ? 0.0f : i % 3 == 0 ? 32.0f : 32.0f * rnd();
    VC[4 * i + 3] = 0.0f;
    feat[4 * (n + i) + 3] = hit ? 1.0f : 0.0f;
    const int32_t id = hit ? 1 + (int32_t)(i % 7) : 0;
    std::memcpy(&feat[4 * (2 * n + i) + 3], &id, sizeof id);
  }
  const float* c = history ? C.data() : nullptr;
  const float* vc = history ? VC.data() : nullptr;
  std::vector<float> Wp(n), NE(n), vb(4 * n);
  const double sse = pthi::noise_counts_host(n, noise.data(), counts.data(), c, vc, Wp.data(), NE.data(), vb.data());
  (void)pthi::noise_counts_host(n, noise.data(), counts.data(), c, vc, Wp.data(), NE.data(), nullptr);
  if (!(sse == sse)) return 4;  // (a NaN in the estimate: something was read that nobody wrote)
  const std::vector<uint32_t> key = pthi::keys_blend_host(W, R, Wp.data(), NE.data());
  if (key.size() != n) return 5;
  const int caps[3] = {1, (int)((n + 3) / 4), (int)n};
  for (int cap : caps) {
    std::vector<int32_t> list((size_t)cap, -1);
    int above = -1, m = -1;
    pthi::select_threshold_blend_host(W, R, noise.data(), counts.data(), c, vc, 0.05f, cap, list.data(), &above, &m);
    if (m < 0 || m > cap || above < m) return 6;
    for (int i = 0; i < m; ++i)
      if (list[(size_t)i] < 0 || (size_t)list[(size_t)i] >= n || (i > 0 && list[(size_t)i] <= list[(size_t)i - 1])) return 7;
    ++*cases;
  }
  std::vector<float> avg(3 * n), K(4 * PT_HISTORY_KEPT_PLANES * n), VK(4 * n);
  pthi::blend_counts_host(n, S.data(), counts.data(), c, avg.data());
  pthi::capture_counts_host(n, S.data(), feat.data(), noise.data(), counts.data(), c, vc, K.data(), VK.data());
  for (size_t i = 0; i < n; ++i) {  // K0 is the blend and NE; VK is pass A's vb
    if (std::memcmp(&K[4 * i], &avg[3 * i], 3 * sizeof(float)) != 0 || std::memcmp(&K[4 * i + 3], &NE[i], sizeof(float)) != 0) return 8;
    if (std::memcmp(&VK[4 * i], &vb[4 * i], 4 * sizeof(float)) != 0) return 9;
  }
  ptdn::Job j{};
  PtDenoiseOptions opt{};
  opt.levels = 2;
  if (ptdn::resolve(&opt, &j.P, ptdn::kHistorySigmaColor)) return 10;
  j.form = ptdn::Form::HistoryAdaptive;
  j.f = {W, R, S.data(), feat.data(), noise.data(), c, vc};
  std::vector<float> out(3 * n), var_raw(n), var_0(n);
  ptdn::denoise_host(j, counts.data(), out.data(), var_raw.data(), var_0.data());
  ptdn::denoise_host(j, counts.data(), nullptr, var_raw.data(), nullptr);
  ++*cases;
  return 0;
}

int main() {
  const int shapes[3][2] = {{97, 61}, {3, 2}, {257, 5}};
  int cases = 0;
  for (const auto& s : shapes)
    for (int history = 0; history < 2; ++history)
      if (const int rc = run(s[0], s[1], history != 0, &cases)) return rc;
  std::printf("threshold: %d cases\n", cases);
  return 0;
}
