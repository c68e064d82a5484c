// The host side of the history's variance and of the filter over the blend, stand-alone: pt_history.h and pt_denoise.h are plain C++,
// so the system compiler builds this with -fsanitize=address,undefined and tests/test_history_variance_host.py runs it directly.
// Two views of a made-up wall at W x R pixels (argv: W R): capture with variance, the lookup with variance from a camera one pixel to
// the side, the filter over the blend, a second capture.  Every array is exactly as large as the functions may touch, on the heap, so
// an access past an end is reported; the exit status is 0 and one line of sums is printed when nothing was.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pt_denoise.h"
#include "pt_history.h"

static uint32_t g_state = 12345u;
static float rnd() {  // [0, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int W = std::atoi(argv[1]), R = std::atoi(argv[2]);
  if (W < 1 || R < 1) return 2;
  const size_t n = (size_t)W * R;
  const int groups = 4, iters = 4;
  const float samples = (float)iters, Tf = (float)iters, Df = (float)(groups - 1) * Tf;

  PtCamera cam{};
  cam.resolution[0] = W, cam.resolution[1] = R;
  cam.position[0] = 0.25f, cam.position[1] = 0.5f, cam.position[2] = -6.0f;
  cam.view[2] = 1.0f, cam.up[1] = 1.0f, cam.right[0] = -1.0f;
  cam.pixelLength[0] = cam.pixelLength[1] = 0.03125f;

  // the first hits of both views: a wall at depth 8; the second view's pixels land between the first view's (and past its edges)
  std::vector<float> S(3 * n), feat0(12 * n), feat1(12 * n), noise(8 * n);
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
        f[4 * (2 * n + i) + 3] = pthi::bits_float(1 + (int32_t)((x / 3 + y / 2) % 2));                            // two objects in patches
      }
      for (int k = 0; k < 3; ++k) {
        const float s = 4.0f * rnd();
        S[3 * i + k] = s;
        noise[4 * i + k] = s;                                             // prev = S at the last fold
        noise[4 * (n + i) + k] = (s * s) / Tf + (i % 7 ? rnd() : 0.0f);  // q: every seventh pixel has variance 0
      }
    }
  if (n > 4) feat1[4 * (n + 3) + 3] = 0.0f;  // a miss

  std::vector<float> K(12 * n), VK(4 * n), C(4 * n), VC(4 * n), K2(12 * n), VK2(4 * n), out(3 * n), blend(3 * n);
  pthi::capture_host(n, S.data(), feat0.data(), nullptr, samples, K.data());
  pthi::capture_variance_host(n, noise.data(), Tf, Df, samples, nullptr, nullptr, VK.data());
  pthi::Params P{};
  if (pthi::resolve(nullptr, &P)) return 3;
  const uint8_t reject[2] = {0, 0};
  pthi::reproject_variance_host(pthi::make_view(cam, R, 0), K.data(), feat1.data(), reject, 2, P, VK.data(), C.data(), VC.data());
  pthi::blend_host(n, S.data(), samples, C.data(), blend.data());

  ptdn::Job j{};
  j.form = ptdn::Form::History;
  if (ptdn::resolve(nullptr, &j.P, ptdn::kHistorySigmaColor)) return 3;
  j.div.Tf = Tf, j.div.Df = Df, j.div.samples = samples;
  j.f = {W, R, S.data(), feat1.data(), noise.data(), C.data(), VC.data()};
  ptdn::denoise_host(j, nullptr, out.data());

  pthi::capture_host(n, S.data(), feat1.data(), C.data(), samples, K2.data());
  pthi::capture_variance_host(n, noise.data(), Tf, Df, samples, C.data(), VC.data(), VK2.data());

  double sums[4] = {0, 0, 0, 0};
  size_t carried = 0;
  for (size_t i = 0; i < n; ++i) {
    carried += C[4 * i + 3] > 0.0f;
    for (int k = 0; k < 3; ++k) sums[0] += VC[4 * i + k], sums[1] += VK2[4 * i + k], sums[2] += out[3 * i + k], sums[3] += blend[3 * i + k];
  }
  std::printf("%d x %d: %zu carried, sums VC %.9g VK %.9g filtered %.9g blend %.9g\n", W, R, carried, sums[0], sums[1], sums[2], sums[3]);
  return sums[2] == sums[2] ? 0 : 4;  // (a NaN in the filtered image: something was read that nobody wrote)
}
