// The host side of the lookup with the objects' motion (PT_HISTORY_MOTION), stand-alone: pt_history.h is plain C++, so the system
// compiler builds this with -fsanitize=address,undefined and tests/test_history_motion_host.py runs it directly.
// A made-up wall at W x R pixels (argv: W R) of three geoms side by side: the first stands still, the second has moved by a pixel and
// a quarter (its current pixels are where the kept ones were, shifted), the third carries nothing.  The motion table comes from
// pthi::motion_table on geoms with those transforms; the lookup runs in its three kinds.  Every array is exactly as large as the
// functions may touch, on the heap — the table and the kinds have one row per geom and the ids run up to the last geom — so an access
// past an end is reported; the exit status is 0 and one line is printed when nothing was.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pt_history.h"

static void identity(float m[16]) {
  std::memset(m, 0, 16 * sizeof(float));
  m[0] = m[5] = m[10] = m[15] = 1.0f;
}
static PtGeom translated(float tx) {  // column-major: the translation in elements 12 .. 14
  PtGeom g{};
  g.type = PT_GEOM_CUBE;
  identity(g.transform), identity(g.inverseTransform), identity(g.invTranspose);
  g.transform[12] = tx, g.inverseTransform[12] = -tx, g.invTranspose[3] = -tx;
  return g;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int W = std::atoi(argv[1]), R = std::atoi(argv[2]);
  if (W < 1 || R < 1) return 2;
  const size_t n = (size_t)W * R;
  const int num_geoms = 3;

  PtCamera cam{};
  cam.resolution[0] = W, cam.resolution[1] = R;
  cam.position[0] = 0.25f, cam.position[1] = 0.5f, cam.position[2] = -6.0f;
  cam.view[2] = 1.0f, cam.up[1] = 1.0f, cam.right[0] = -1.0f;
  cam.pixelLength[0] = cam.pixelLength[1] = 0.03125f;
  const float depth = 8.0f, shift_px = 1.25f, shift = shift_px * depth * cam.pixelLength[0];  // world units per pixel at this depth: 0.25

  std::vector<PtGeom> kept{translated(0.0f), translated(1.0f), PtGeom{}}, cur{translated(0.0f), translated(1.0f + shift), PtGeom{}};
  kept[2].type = cur[2].type = PT_GEOM_TRIANGLE;
  kept[2].transform[0] = 1.0f, cur[2].transform[0] = 2.0f;  // a changed vertex word
  std::vector<float> table((size_t)num_geoms * pthi::kMotionRow);
  std::vector<uint8_t> kind((size_t)num_geoms);
  pthi::motion_table(kept.data(), cur.data(), num_geoms, table.data(), kind.data());
  if (kind[0] != pthi::kStill || kind[1] != pthi::kMoved || kind[2] != pthi::kCarriesNothing) return 6;

  // the kept planes: every pixel its own point of the wall (pixel x looks along sx = x: generateRayFromCamera); the current feature sums: the same points, the second geom's shifted
  std::vector<float> K(12 * n), VK(4 * n), feat(12 * n);
  for (int y = 0; y < R; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t i = (size_t)y * W + x;
      const int32_t id = 1 + (3 * x) / W;  // 1 .. 3 from left to right
      const float px = cam.position[0] - ((float)W * 0.5f - (float)x) * depth * cam.pixelLength[0];
      const float py = cam.position[1] + ((float)R * 0.5f - (float)y) * depth * cam.pixelLength[1];
      K[4 * i] = (float)x, K[4 * i + 1] = (float)y, K[4 * i + 2] = 0.5f, K[4 * i + 3] = 4.0f;
      K[4 * (n + i)] = px, K[4 * (n + i) + 1] = py, K[4 * (n + i) + 2] = cam.position[2] + depth, K[4 * (n + i) + 3] = pthi::bits_float(id);
      K[4 * (2 * n + i) + 2] = -1.0f;
      VK[4 * i] = VK[4 * i + 1] = VK[4 * i + 2] = 0.125f, VK[4 * i + 3] = 0.25f;
      feat[4 * i + 2] = -1.0f;
      feat[4 * (n + i)] = feat[4 * (n + i) + 1] = feat[4 * (n + i) + 2] = 0.5f, feat[4 * (n + i) + 3] = 1.0f;
      feat[4 * (2 * n + i)] = px + (id == 2 ? shift : 0.0f), feat[4 * (2 * n + i) + 1] = py, feat[4 * (2 * n + i) + 2] = cam.position[2] + depth;
      feat[4 * (2 * n + i) + 3] = pthi::bits_float(id);
    }
  if (n > 4) feat[4 * (n + 3) + 3] = 0.0f;  // a miss

  pthi::Params P{};
  if (pthi::resolve(nullptr, &P)) return 3;
  const std::vector<uint8_t> reject((size_t)num_geoms, 0);
  const pthi::Motion mo{table.data(), kind.data()};
  const pthi::View v = pthi::make_view(cam, R, 0);
  std::vector<float> C0(4 * n), C1(4 * n), VC1(4 * n), C2(4 * n), VC2(4 * n), plain(4 * n);
  pthi::reproject_motion_host<pthi::kPlain>(v, K.data(), feat.data(), reject.data(), num_geoms, P, nullptr, mo, C0.data(), nullptr);
  pthi::reproject_motion_host<pthi::kVariance>(v, K.data(), feat.data(), reject.data(), num_geoms, P, VK.data(), mo, C1.data(), VC1.data());
  pthi::reproject_motion_host<pthi::kMoments>(v, K.data(), feat.data(), reject.data(), num_geoms, P, VK.data(), mo, C2.data(), VC2.data());
  pthi::reproject_host(v, K.data(), feat.data(), reject.data(), num_geoms, P, plain.data());

  // the moved geom's pixels find their own kept pixel again (the plain lookup finds the one 1.25 pixels to the side); the third geom's carry nothing
  size_t carried[3] = {0, 0, 0}, pixels[3] = {0, 0, 0}, exact = 0;
  for (size_t i = 0; i < n; ++i) {
    if (std::memcmp(&C0[4 * i], &C1[4 * i], 16) || std::memcmp(&C0[4 * i], &C2[4 * i], 16)) return 7;  // C does not depend on the kind
    if (!(feat[4 * (n + i) + 3] > 0.0f)) continue;
    const int g = pthi::float_bits(feat[4 * (2 * n + i) + 3]) - 1;
    pixels[g] += 1;
    carried[g] += C0[4 * i + 3] > 0.0f ? 1 : 0;
    if (g == 1 && C0[4 * i + 3] > 0.0f && C0[4 * i] == K[4 * i]) exact += 1;
    if (g == 0 && std::memcmp(&C0[4 * i], &plain[4 * i], 16)) return 8;  // a still geom: the plain lookup's value
  }
  if (carried[2] != 0) return 9;
  std::printf("%d x %d: carried %zu of %zu still, %zu of %zu moved (%zu on their own kept pixel), %zu of %zu changed triangle\n", W, R, carried[0], pixels[0],
              carried[1], pixels[1], exact, carried[2], pixels[2]);
  return 0;
}
