// The host side of the lookup with the materials' edits (PT_HISTORY_MATERIALS), stand-alone: pt_history.h is plain C++, so the system
// compiler builds this with -fsanitize=address,undefined and tests/test_history_materials_host.py runs it directly.
// A made-up wall at W x R pixels (argv: W R) of three geoms side by side, each with a material of its own: the first is unchanged, the
// second recoloured (its colour doubled, halved and kept), the third became an emitter and carries nothing.  The recolour table comes
// from pthi::recolor_table; the lookup runs in its three kinds, without a motion table and with one in which every geom is still.
// Every array is exactly as large as the functions may touch, on the heap — the tables and the kinds have one row per geom and the
// ids run up to the last geom — so an access past an end is reported; the exit status is 0 and one line is printed when nothing was.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pt_history.h"

static PtMaterial diffuse(float r, float g, float b) {
  PtMaterial m{};
  m.color[0] = r, m.color[1] = g, m.color[2] = b;
  return m;
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
  const float depth = 8.0f;

  std::vector<PtGeom> geoms((size_t)num_geoms);
  for (int g = 0; g < num_geoms; ++g) geoms[(size_t)g].type = PT_GEOM_CUBE, geoms[(size_t)g].materialid = g;
  std::vector<PtMaterial> kept{diffuse(0.5f, 0.5f, 0.5f), diffuse(0.25f, 0.5f, 0.75f), diffuse(0.5f, 0.5f, 0.5f)}, cur = kept;
  cur[1] = diffuse(0.5f, 0.25f, 0.75f);
  cur[2].emittance = 5.0f;
  std::vector<float> recolor((size_t)num_geoms * pthi::kRecolorRow);
  std::vector<uint8_t> rkind((size_t)num_geoms);
  pthi::recolor_table(kept.data(), cur.data(), num_geoms, geoms.data(), num_geoms, recolor.data(), rkind.data());
  if (rkind[0] != pthi::kUnchanged || rkind[1] != pthi::kRecolored || rkind[2] != pthi::kCarriesNothing) return 6;
  if (recolor[4] != 2.0f || recolor[5] != 0.5f || recolor[6] != 1.0f || recolor[7] != 0.0f) return 6;
  std::vector<float> table((size_t)num_geoms * pthi::kMotionRow);
  std::vector<uint8_t> kind((size_t)num_geoms);
  pthi::motion_table(geoms.data(), geoms.data(), num_geoms, table.data(), kind.data());

  // the kept planes: every pixel its own point of the wall; the current feature sums: the same points
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
      feat[4 * (2 * n + i)] = px, feat[4 * (2 * n + i) + 1] = py, feat[4 * (2 * n + i) + 2] = cam.position[2] + depth;
      feat[4 * (2 * n + i) + 3] = pthi::bits_float(id);
    }
  if (n > 4) feat[4 * (n + 3) + 3] = 0.0f;  // a miss

  pthi::Params P{};
  if (pthi::resolve(nullptr, &P)) return 3;
  const std::vector<uint8_t> reject((size_t)num_geoms, 0);
  const pthi::Motion mo{table.data(), kind.data()};
  const pthi::Recolor rc{recolor.data(), rkind.data()};
  const pthi::View v = pthi::make_view(cam, R, 0);
  std::vector<float> C0(4 * n), C1(4 * n), VC1(4 * n), C2(4 * n), VC2(4 * n), C3(4 * n), VC3(4 * n), plain(4 * n), VP(4 * n);
  pthi::reproject_materials_host<pthi::kPlain>(v, K.data(), feat.data(), reject.data(), num_geoms, P, nullptr, nullptr, rc, C0.data(), nullptr);
  pthi::reproject_materials_host<pthi::kVariance>(v, K.data(), feat.data(), reject.data(), num_geoms, P, VK.data(), nullptr, rc, C1.data(), VC1.data());
  pthi::reproject_materials_host<pthi::kMoments>(v, K.data(), feat.data(), reject.data(), num_geoms, P, VK.data(), nullptr, rc, C2.data(), VC2.data());
  pthi::reproject_materials_host<pthi::kMoments>(v, K.data(), feat.data(), reject.data(), num_geoms, P, VK.data(), &mo, rc, C3.data(), VC3.data());
  pthi::reproject_moments_host(v, K.data(), feat.data(), reject.data(), num_geoms, P, VK.data(), plain.data(), VP.data());

  size_t scaled = 0, pixels[3] = {0, 0, 0};
  for (size_t i = 0; i < n; ++i) {
    if (std::memcmp(&C0[4 * i], &C1[4 * i], 16) || std::memcmp(&C0[4 * i], &C2[4 * i], 16)) return 7;  // C does not depend on the kind
    if (std::memcmp(&C2[4 * i], &C3[4 * i], 16) || std::memcmp(&VC2[4 * i], &VC3[4 * i], 16)) return 7;  // ... nor on a table of still geoms
    if (!(feat[4 * (n + i) + 3] > 0.0f)) continue;
    const int g = pthi::float_bits(feat[4 * (2 * n + i) + 3]) - 1;
    pixels[g] += 1;
    if (g == 0 && (std::memcmp(&C2[4 * i], &plain[4 * i], 16) || std::memcmp(&VC2[4 * i], &VP[4 * i], 16))) return 8;  // unchanged: the lookup without the flag
    if (g == 2 && (C2[4 * i + 3] != 0.0f || VC2[4 * i] != 0.0f)) return 9;                                               // carries nothing
    if (g == 1) {
      if (C2[4 * i] != plain[4 * i] * 2.0f || C2[4 * i + 1] != plain[4 * i + 1] * 0.5f || C2[4 * i + 2] != plain[4 * i + 2] || C2[4 * i + 3] != plain[4 * i + 3]) return 10;
      if (VC2[4 * i] != VP[4 * i] * 4.0f || VC2[4 * i + 1] != VP[4 * i + 1] * 0.25f || VC2[4 * i + 3] != VP[4 * i + 3]) return 11;
      if (VC1[4 * i + 3] != 0.0f) return 12;
      scaled += C2[4 * i + 3] > 0.0f ? 1 : 0;
    }
  }
  std::printf("%d x %d: scaled %zu of %zu recoloured pixels; %zu unchanged, %zu that carry nothing\n", W, R, scaled, pixels[1], pixels[0], pixels[2]);
  return 0;
}
