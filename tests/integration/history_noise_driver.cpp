// The host side of the noise estimate of the blend, stand-alone: pt_noise.h and pt_history.h are plain C++, so the system compiler builds
// this with -fsanitize=address,undefined and tests/test_history_noise_host.py runs it directly.  A made-up render of `pixels` pixels
// (argv: pixels) in three folded groups, the estimate after the second and third fold with the history absent and present.  Every array
// is exactly as large as the functions may touch, on the heap, so an access past an end is reported; the exit status is 0 and one line
// of sums is printed when nothing was.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pt_history.h"
#include "pt_noise.h"

static uint32_t g_state = 2463534242u;
static float rnd() {  // [0, 1)
  g_state = g_state * 1664525u + 1013904223u;
  return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const int pixels = std::atoi(argv[1]);
  if (pixels < 1) return 2;
  const size_t n = (size_t)pixels;
  std::vector<float> S(3 * n, 0.0f), planes(4 * PT_NOISE_PLANES * n, 0.0f), C(4 * n), VC(4 * n), W(n), W0(n);
  for (size_t i = 0; i < n; ++i) {
    const bool gone = i % 4 == 3;  // a rejected pixel: all zero
    for (int k = 0; k < 3; ++k) C[4 * i + k] = gone ? 0.0f : rnd(), VC[4 * i + k] = gone || i % 5 == 0 ? 0.0f : rnd() * 0.01f;
    C[4 * i + 3] = gone ? 0.0f : i % 3 == 0 ? 32.0f : 32.0f * rnd();
    VC[4 * i + 3] = 0.0f;
  }
  const int group[3] = {3, 1, 4};
  int64_t T = 0;
  double sums[3] = {0, 0, 0};
  size_t same = 0;
  for (int M = 1; M <= 3; ++M) {
    for (int s = 0; s < group[M - 1]; ++s)
      for (size_t j = 0; j < 3 * n; ++j) S[j] += (j / 3) % 7 ? 2.0f * rnd() : 0.5f;  // every seventh pixel is constant
    T += group[M - 1];
    const ptnz::Fold f = ptnz::fold_scalars(group[M - 1], M, T);
    const double view = ptnz::fold_host(n, S.data(), planes.data(), f);
    if (M < 2) continue;
    const double absent = pthi::noise_host(n, planes.data(), f.Tf, f.Df, f.Tf, nullptr, nullptr, W0.data());
    const double blend = pthi::noise_host(n, planes.data(), f.Tf, f.Df, f.Tf, C.data(), VC.data(), W.data());
    (void)pthi::noise_host(n, planes.data(), f.Tf, f.Df, f.Tf, C.data(), VC.data(), nullptr);
    // the history absent: the fold's own plane-0 .w and its double, bit for bit
    for (size_t i = 0; i < n; ++i) same += std::memcmp(&W0[i], &planes[4 * i + 3], sizeof(float)) == 0;
    if (std::memcmp(&absent, &view, sizeof(double)) != 0) return 5;
    sums[0] = view, sums[1] = absent, sums[2] = blend;
  }
  if (same != 2 * n) return 6;
  std::printf("%d pixels: %zu words equal the fold's, sums view %.17g absent %.17g blend %.17g\n", pixels, same, sums[0], sums[1], sums[2]);
  return sums[2] == sums[2] ? 0 : 4;  // (a NaN in the estimate: something was read that nobody wrote)
}
