// Prints csrc/pt_lds.h's byte maps for a sweep of scene sizes (tests/test_lds_layout.py compiles this with the system
// compiler, runs it and checks the maps).  Output: `name key=value ...` lines for the constants and the per-wave maps,
// then one `case` line per swept SceneTables, each followed by one line per (kernel map, form).
#include <cstdio>

#include "pt_lds.h"

using namespace ptk;

static void put(const char* name, const LegacyLds& L) { printf("%s nodes=%d geoms=%d total=%d\n", name, L.nodes, L.geoms, L.total); }
static void put(const char* name, const IntersectLds& L) {
  printf("%s top=%d nodes=%d geoms=%d waves=%d wave_bytes=%d total=%d\n", name, L.top, L.nodes, L.geoms, L.waves, L.wave_bytes, L.total);
}
static void put(const char* name, const IntersectGridLds& L) { printf("%s waves=%d wave_bytes=%d total=%d\n", name, L.waves, L.wave_bytes, L.total); }
static void put(const char* name, const PrimaryLds& L) {
  printf("%s top=%d mats=%d nodes=%d geoms=%d waves=%d wave_bytes=%d ihash=%d cam_top=%d cam_qo=%d total=%d\n", name, L.top, L.mats, L.nodes,
         L.geoms, L.waves, L.wave_bytes, L.ihash, L.cam_top, L.cam_qo, L.total);
}
static void put(const char* name, const PathsLds& L) {
  printf("%s top=%d mats=%d geoms=%d nodes=%d waves=%d wave_bytes=%d tword=%d lmat=%d ihash=%d total=%d\n", name, L.top, L.mats, L.geoms,
         L.nodes, L.waves, L.wave_bytes, L.tword, L.lmat, L.ihash, L.total);
}
static void put(const char* name, const ShadeLds& L) { printf("%s mats=%d ihash=%d total=%d\n", name, L.mats, L.ihash, L.total); }

template <bool SMALL, int NPAR>
static void put_carry(const char* name) {
  using M = CarryMap<SMALL, NPAR>;
  printf("%s best=%d rec=%d ray=%d ent=%d slot=%d bytes=%d\n", name, M::best, M::rec, M::ray, M::ent, M::slot, M::bytes);
}
template <bool FAST, bool EX>
static void put_grid(const char* name) {
  using M = GridMap<FAST, EX>;
  printf("%s cells=%d gix=%d rinv=%d bytes=%d planes=%d\n", name, M::cells, M::gix, M::rinv, M::bytes, rinv_planes<FAST, EX>());
}
template <Search F, bool FAST>
static void put_paths_wave(const char* name) {
  using M = PathsWaveMap<F, FAST>;
  printf("%s slots=%d died=%d fillc=%d bytes=%d\n", name, M::slots, M::died, M::fillc, M::bytes);
}

// every map of one arithmetic flavour (FAST: the fast build; depth 0 then runs the exact arithmetic, EX, as in the fma build)
template <bool FAST, bool EX>
static void put_case(const SceneTables& sc) {
  put("legacy.0", legacy_lds<false>(sc));
  put("legacy.1", legacy_lds<true>(sc));
  put("intersect.0", intersect_lds<false>(sc));
  put("intersect.1", intersect_lds<true>(sc));
  put("intersect_grid.primary", intersect_grid_lds<FAST, EX>(sc));  // the stage kernel's two forms: depth 0 (EX) and bounce
  put("intersect_grid.bounce", intersect_grid_lds<FAST, false>(sc));
  put("primary.lds", primary_lds<kLdsTables, FAST, EX>(sc));
  put("primary.scan", primary_lds<kTopScan, FAST, EX>(sc));
  put("primary.grid", primary_lds<kGrid, FAST, EX>(sc));
  put("paths.lds", paths_lds<kLdsTables, FAST>(sc));
  put("paths.scan", paths_lds<kTopScan, FAST>(sc));
  put("paths.grid", paths_lds<kGrid, FAST>(sc));
  put("shade", shade_lds<true>(sc));
  put("shade_stage", shade_lds<false>(sc));
}

int main() {
  printf("sizes Mat=%d Node=%d Geom=%d TopEntry=%d kMaxTop=%d kIterHashMax=%d kWavesPerBlock=%d kCandCap=%d kRing=%d kCellRing=%d kVisitRing=%d "
         "kSlotTail=%d kSlotVisit=%d kSlotBytes=%d\n",
         (int)sizeof(ptd::Mat), (int)sizeof(ptd::Node), (int)sizeof(ptd::Geom), (int)sizeof(ptd::TopEntry), kMaxTop, kIterHashMax, kWavesPerBlock,
         kCandCap, kRing, kCellRing, kVisitRing, kSlotTail, kSlotVisit, kSlotBytes);
  printf("wave.WaveMap best=%d rec=%d list=%d bytes=%d\n", WaveMap::best, WaveMap::rec, WaveMap::list, WaveMap::bytes);
  printf("wave.LanesMap best=%d rec=%d ent=%d bytes=%d\n", LanesMap::best, LanesMap::rec, LanesMap::ent, LanesMap::bytes);
  put_carry<true, 2>("wave.CarryMap.small.2");
  put_carry<false, 1>("wave.CarryMap.full.1");
  put_carry<false, 2>("wave.CarryMap.full.2");
  put_grid<false, false>("wave.GridMap.fast0.ex0");
  put_grid<false, true>("wave.GridMap.fast0.ex1");
  put_grid<true, false>("wave.GridMap.fast1.ex0");
  put_grid<true, true>("wave.GridMap.fast1.ex1");
  put_paths_wave<kLdsTables, false>("wave.PathsWaveMap.lds.fast0");
  put_paths_wave<kTopScan, false>("wave.PathsWaveMap.scan.fast0");
  put_paths_wave<kGrid, false>("wave.PathsWaveMap.grid.fast0");
  put_paths_wave<kLdsTables, true>("wave.PathsWaveMap.lds.fast1");
  put_paths_wave<kTopScan, true>("wave.PathsWaveMap.scan.fast1");
  put_paths_wave<kGrid, true>("wave.PathsWaveMap.grid.fast1");

  const int sizes[][2] = {{7, 13}, {64, 127}, {156, 311}, {1000, 1999}, {5000, 9999}};  // geoms, nodes: cornell.txt to a few thousand
  const int mats[] = {1, 2, 7, 33, 1000};
  const int iters[] = {1, 25, kIterHashMax - 1, kIterHashMax, kIterHashMax + 1, 1000};
  const int depths[] = {1, 2, 8, 64};
  for (int top = 1; top <= kMaxTop; ++top)
    for (const auto& gn : sizes)
      for (int m : mats)
        for (int it : iters)
          for (int depth : depths) {
            // the full product for a few top-list lengths, every length on the diagonal of the other axes
            const bool corner = top == 1 || top == 2 || top == 7 || top == kMaxTop - 1 || top == kMaxTop;
            if (!corner && !((gn[0] == 7 && m == 7 && depth == 8) || (gn[0] == 156 && m == 33 && it == 25))) continue;
            for (int scan = 0; scan <= 1; ++scan)
              for (int fast = 0; fast <= 1; ++fast) {
                SceneTables sc{};
                sc.num_top = top, sc.num_geoms = gn[0], sc.num_nodes = gn[1], sc.num_mats = m;
                sc.max_batch_iters = it, sc.trace_depth = depth, sc.scan_nodes_lds = scan;
                printf("case top=%d geoms=%d nodes=%d mats=%d iters=%d depth=%d scan=%d fast=%d\n", top, gn[0], gn[1], m, it, depth, scan, fast);
                if (fast) put_case<true, true>(sc);
                else put_case<false, false>(sc);
              }
          }
  return 0;
}
