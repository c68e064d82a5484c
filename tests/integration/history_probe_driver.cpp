// The host side of the history probes, stand-alone: pt_history.h is plain C++, so the system compiler builds this with
// -fsanitize=address,undefined and tests/test_history_probe_host.py runs it directly.
// A made-up tile of W x R pixels (argv: W R) of four objects side by side with a miss and an id past the table; at each of the nine
// phases: the list, the keep, a replay that differs at every fifth probe, the gradient with one geom moved, and the apply at radius
// 0 .. 4.  Every array is exactly as large as the functions may touch, on the heap, so an access past an end is reported; the exit
// status is 0 and one line is printed when nothing was.
#include <cstdio>
#include <cstdlib>
#include <vector>

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
  const int num_geoms = 4;
  const uint8_t moved[num_geoms] = {0, 0, 1, 0};

  std::vector<float> S(3 * n), feat(12 * n), C(4 * n);
  for (float& x : S) x = 4.0f * rnd();
  for (float& x : feat) x = rnd();
  for (float& x : C) x = 8.0f * rnd();
  for (size_t i = 0; i < n; ++i) {
    feat[4 * (n + i) + 3] = 1.0f;
    feat[4 * (2 * n + i) + 3] = pthi::bits_float(1 + (int32_t)(4 * (i % (size_t)W) / (size_t)W));
  }
  if (n > 4) feat[4 * (n + 3) + 3] = 0.0f;                                // a miss
  if (n > 6) feat[4 * (2 * n + 5) + 3] = pthi::bits_float(num_geoms + 1);  // an id past the table

  long changed_all = 0, skipped_all = 0, probes_all = 0;
  double sum = 0.0;
  for (int phase = 0; phase < 9; ++phase) {
    const pthi::ProbeGrid pg = pthi::probe_grid(W, R, phase);
    const int P = pthi::probe_count(pg);
    if (P < 0 || (size_t)P > n) return 5;
    std::vector<int32_t> list((size_t)P);
    for (int s = 0; s < P; ++s) {
      list[(size_t)s] = pthi::probe_pixel(pg, W, s);
      if (list[(size_t)s] < 0 || (size_t)list[(size_t)s] >= n || (s > 0 && list[(size_t)s] <= list[(size_t)s - 1])) return 6;
    }
    std::vector<float> PK(4 * (size_t)P), Sw(3 * (size_t)P), L((size_t)P);  // exactly P entries: nothing reads or writes further
    pthi::probe_keep_host(W, R, phase, S.data(), feat.data(), PK.data());
    for (int s = 0; s < P; ++s)
      for (int k = 0; k < 3; ++k) Sw[3 * (size_t)s + k] = PK[4 * (size_t)s + k] + (s % 5 == 0 ? 0.25f * rnd() : 0.0f);
    int changed = -1, skipped = -1;
    pthi::probe_gradient_host(W, R, phase, PK.data(), Sw.data(), feat.data(), moved, num_geoms, L.data(), &changed, &skipped);
    if (changed < 0 || skipped < 0 || changed + skipped > P) return 7;
    for (int radius = 0; radius <= 4; ++radius) {
      PtHistoryProbeOptions o{};
      o.radius = radius ? radius : -1, o.gain = radius == 2 ? 2.0f : 0.0f;
      pthi::ProbeParams pp{};
      if (pthi::resolve_probe(&o, &pp) || pp.radius != radius) return 3;
      std::vector<float> c = C;
      pthi::probe_apply_host(W, R, phase, L.data(), feat.data(), moved, num_geoms, pp, c.data());
      for (float x : c) sum += x;
    }
    changed_all += changed, skipped_all += skipped, probes_all += P;
  }
  if ((size_t)probes_all != n) return 8;  // the nine phases cover the tile once
  std::printf("%d x %d, 9 phases, %ld probes, changed: %ld skipped: %ld, sum %.9g\n", W, R, probes_all, changed_all, skipped_all, sum);
  return sum == sum ? 0 : 4;  // (a NaN: something was read that nobody wrote)
}
