// pt_lds.h — the dynamic-LDS byte maps of the traversal and shading kernels, one per kernel family.
//
// A kernel takes every LDS pointer from its map and the launch code (pt_launch.inc) requests the map's `total`, so the
// two cannot disagree.  Plain C++ (the system compiler accepts it; tests/test_lds_layout.py sweeps every map): offsets
// only — the pointer structs that sit on the per-wave blocks (WaveLds, Carry, Lanes, CellRing) and their *_init
// functions are in pt_kernels.hip / pt_grid.inc and take their offsets from the *Map structs below.
#pragma once
#include "pt_kernels.h"

namespace ptk {

// Regions follow each other without padding and are staged / read with 16-byte accesses: every table record is a
// multiple of 16 bytes (only the materials' end is rounded: what follows them differs by kernel).
static_assert(sizeof(ptd::Mat) % 16 == 0 && sizeof(ptd::Node) % 16 == 0 && sizeof(ptd::Geom) % 16 == 0 &&
                  sizeof(ptd::TopEntry) % 16 == 0,
              "the LDS maps place the scene tables back to back and copy them 16 bytes at a time");
__host__ __device__ constexpr int round16(int x) { return (x + 15) & ~15; }

__host__ __device__ inline int top_bytes(const SceneTables& sc) { return sc.num_top * (int)sizeof(ptd::TopEntry); }
__host__ __device__ inline int mat_bytes(const SceneTables& sc) { return round16(sc.num_mats * (int)sizeof(ptd::Mat)); }
__host__ __device__ inline int node_bytes(const SceneTables& sc) { return sc.num_nodes * (int)sizeof(ptd::Node); }
__host__ __device__ inline int geom_bytes(const SceneTables& sc) { return sc.num_geoms * (int)sizeof(ptd::Geom); }
__host__ __device__ inline int table_bytes(const SceneTables& sc) { return node_bytes(sc) + geom_bytes(sc); }
__host__ __device__ inline bool tables_in_lds(const SceneTables& sc) { return table_bytes(sc) <= sc.lds_table_bytes; }

// How the fused kernels (k_primary, k_paths) find a ray's candidate leaves.
enum Search {
  kLdsTables = 0,  // scene tables in LDS, every leaf a top-list entry (cornell.txt)
  kTopScan = 1,    // tables in memory: top list + per-lane subtree scans (k_paths) / one packet scan per group (k_primary)
  kGrid = 2,       // tables in memory: uniform grid walk
};
__host__ __device__ inline Search search_form(const SceneTables& sc) {
  return sc.use_grid ? kGrid : tables_in_lds(sc) ? kLdsTables : kTopScan;
}

// Per-iteration RNG hash table (pt_kernels.hip iter_hash_fill): the context's iterations per batch
// (SceneTables::max_batch_iters) in whole 16 bytes, none beyond kIterHashMax (larger batches hash per ray).
constexpr int kIterHashMax = 256;
__host__ __device__ inline int iter_hash_entries(const SceneTables& sc) {
  return sc.max_batch_iters <= kIterHashMax ? (sc.max_batch_iters + 3) & ~3 : 0;
}

// ── per-wave blocks ───────────────────────────────────────────────────────────────────────────────────────────────────
constexpr int kCandCap = 192;  // per-wave candidate list entries of the per-group search (WaveLds::list)
struct WaveMap {               // WaveLds: best keys [64] x 8 B, winner records + donor row [7][64] x 4 B, candidate list
  static constexpr int best = 0, rec = best + 64 * 8, list = rec + 7 * 64 * 4, bytes = list + kCandCap * 4;  // 3072 B
};
constexpr int kRing = 128;  // candidate-ring entries per wave (power of two; <= 63 pending + <= 64 appended at once)
template <bool SMALL, int NPAR>
struct CarryMap {  // Carry<SMALL, NPAR>: keys, records, rays (SMALL: directions only), ring (SMALL: 16-bit entries), steal scratch (not SMALL)
  static constexpr int best = 0, rec = best + NPAR * 64 * 8, ray = rec + NPAR * 6 * 64 * 4, ent = ray + NPAR * (SMALL ? 3 : 6) * 64 * 4,
                       slot = ent + kRing * (SMALL ? 2 : 4), bytes = slot + (SMALL ? 0 : 64 * 4);
};
struct LanesMap {  // Lanes (k_paths, tables in LDS): keys, records, 16-bit ring
  static constexpr int best = 0, rec = best + 64 * 8, ent = rec + 6 * 64 * 4, bytes = ent + kRing * 2;
};
// The grid walk's block: a Carry<false, 1>, then the cell ring, Carry::gix and CellRing::rinv.  rinv holds the reciprocal
// direction of each lane's ray and, where the slab test has the FMA form (the fast build's bounce rays), -origin * that.
constexpr int kCellRing = 256;  // entries (power of two): what is left of a step (< 64) + what a step files (<= 192 at once)
template <bool FAST, bool EX>
constexpr int rinv_planes() { return (EX || !FAST) ? 3 : 6; }
template <bool FAST, bool EX>
struct GridMap {
  static constexpr int cells = CarryMap<false, 1>::bytes, gix = cells + kCellRing * 4, rinv = gix + kRing * 4,
                       bytes = rinv + rinv_planes<FAST, EX>() * 64 * 4;
};
// k_paths: the search form's block, then (tables in LDS only) the lanes' refill slots — planes 0 and 1 of the next path
// record (16 B per lane each), colour.z, sample id, visit: the targets of global_load_lds_dwordx4 / _dword — the 64
// counters of paths retired per depth and the visit ring.
constexpr int kSlotTail = 2 * 64 * 16, kSlotVisit = kSlotTail + 2 * 64 * 4, kSlotBytes = kSlotVisit + 64 * 4;
constexpr int kVisitRing = 64;
template <Search F, bool FAST>
struct PathsWaveMap {
  static constexpr int slots = F == kLdsTables ? LanesMap::bytes : F == kTopScan ? CarryMap<false, 1>::bytes : GridMap<FAST, false>::bytes,
                       died = slots + (F == kLdsTables ? kSlotBytes : 0), fillc = died + 64 * 4, bytes = fillc + kVisitRing * 4;
};

// ── per-workgroup maps ────────────────────────────────────────────────────────────────────────────────────────────────
// Every member but wave_bytes / total is the byte offset of a region; a region ends where the next one starts (an
// absent one is empty), `waves` holds kWavesPerBlock blocks of wave_bytes, total is the end of the last region.
struct LegacyLds {  // k_intersect_legacy
  int nodes, geoms, total;
};
template <bool TABLES_IN_LDS>
__host__ __device__ inline LegacyLds legacy_lds(const SceneTables& sc) {
  LegacyLds L;
  L.nodes = 0;
  L.geoms = L.nodes + (TABLES_IN_LDS ? node_bytes(sc) : 0);
  L.total = L.geoms + (TABLES_IN_LDS ? geom_bytes(sc) : 0);
  return L;
}

struct IntersectLds {  // k_intersect
  int top, nodes, geoms, waves, wave_bytes, total;
};
template <bool TABLES_IN_LDS>
__host__ __device__ inline IntersectLds intersect_lds(const SceneTables& sc) {
  IntersectLds L;
  L.top = 0;
  L.nodes = L.top + top_bytes(sc);
  L.geoms = L.nodes + (TABLES_IN_LDS ? node_bytes(sc) : 0);
  L.waves = L.nodes + (TABLES_IN_LDS ? table_bytes(sc) : 0);
  L.wave_bytes = WaveMap::bytes;
  L.total = L.waves + kWavesPerBlock * L.wave_bytes;
  return L;
}

struct IntersectGridLds {  // k_intersect_grid: the waves' grid blocks alone (the walk reads every table from memory)
  int waves, wave_bytes, total;
};
template <bool FAST, bool EX>
__host__ __device__ inline IntersectGridLds intersect_grid_lds(const SceneTables&) {
  IntersectGridLds L;
  L.waves = 0;
  L.wave_bytes = GridMap<FAST, EX>::bytes;
  L.total = L.waves + kWavesPerBlock * L.wave_bytes;
  return L;
}

struct PrimaryLds {  // k_primary; cam_top / cam_qo: camera-relative copies of the top list / the camera in every geom's object space
  int top, mats, nodes, geoms, waves, wave_bytes, ihash, cam_top, cam_qo, total;
};
template <Search F, bool FAST, bool EX>
__host__ __device__ inline PrimaryLds primary_lds(const SceneTables& sc) {
  PrimaryLds L;
  L.top = 0;
  L.mats = L.top + (F == kGrid ? 0 : top_bytes(sc));
  L.nodes = L.mats + mat_bytes(sc);
  L.geoms = L.nodes + (F == kLdsTables ? node_bytes(sc) : 0);
  L.waves = L.nodes + (F == kLdsTables ? table_bytes(sc) : 0);
  L.wave_bytes = F == kGrid ? GridMap<FAST, EX>::bytes : F == kLdsTables ? CarryMap<true, 2>::bytes : WaveMap::bytes;
  L.ihash = L.waves + kWavesPerBlock * L.wave_bytes;
  L.cam_top = L.ihash + iter_hash_entries(sc) * 4;
  L.cam_qo = L.cam_top + (F == kGrid ? 0 : top_bytes(sc));
  L.total = L.cam_qo + (F == kLdsTables ? round16(sc.num_geoms * 12) : 0);
  return L;
}

struct PathsLds {  // k_paths; tword / lmat: per top entry leaf | geom << 8, per leaf its material; ihash: one row per depth 1 .. trace_depth - 1
  int top, mats, geoms, nodes, waves, wave_bytes, tword, lmat, ihash, total;
};
template <Search F, bool FAST>
__host__ __device__ inline PathsLds paths_lds(const SceneTables& sc) {
  PathsLds L;
  L.top = 0;
  L.mats = L.top + (F == kGrid ? 0 : top_bytes(sc));
  L.geoms = L.mats + mat_bytes(sc);
  L.nodes = L.geoms + (F == kLdsTables ? geom_bytes(sc) : 0);
  L.waves = L.nodes + (F == kTopScan && sc.scan_nodes_lds > 0 ? node_bytes(sc) : 0);
  L.wave_bytes = PathsWaveMap<F, FAST>::bytes;
  L.tword = L.waves + kWavesPerBlock * L.wave_bytes;
  L.lmat = L.tword + (F == kLdsTables ? kMaxTop * 4 : 0);
  L.ihash = L.lmat + (F == kLdsTables ? 64 * 4 : 0);
  L.total = L.ihash + iter_hash_entries(sc) * 4 * (sc.trace_depth > 1 ? sc.trace_depth - 1 : 0);
  return L;
}

struct ShadeLds {  // k_shade (IHASH) and k_shade_stage
  int mats, ihash, total;
};
template <bool IHASH>
__host__ __device__ inline ShadeLds shade_lds(const SceneTables& sc) {
  ShadeLds L;
  L.mats = 0;
  L.ihash = L.mats + mat_bytes(sc);
  L.total = L.ihash + (IHASH ? iter_hash_entries(sc) * 4 : 0);
  return L;
}

}  // namespace ptk
