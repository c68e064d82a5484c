// pt_tables.h — the scene tables the renderer uploads, built on the host from a PtSceneDesc.  Plain C++, no HIP:
// pt_api.cpp uploads them, and its host-only helpers pt_traversal_boxes / pt_build_grid call the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/pt_amd.h"
#include "pt_device.h"

namespace pt {

constexpr int kGridNodes = 600;  // scenes from this many BVH nodes on are candidates for the uniform grid (build_grid, choose_traversal); the ladder scene of 500 primitives (999 nodes): scan 3.9 k, grid 4.7 k Msamples/s, 156 primitives (311 nodes): 5.5 / 5.3
constexpr int kTightNodes = 64;  // scenes from this many BVH nodes on test sphere leaves against the ellipsoid's box (sphere_tight_box); the
                                 // reference's own scenes (cornell.txt: 13 nodes) keep the reference's boxes

struct ThreadedBvh {             // buildBVH's tree (`ref`) re-emitted in visiting order (`nodes`, ptd::Node)
  std::vector<PtBVHNode> ref;
  std::vector<ptd::Node> nodes;
  std::vector<int> where;        // index in `nodes` of reference node i
};
ThreadedBvh threaded_bvh(const PtGeom* geoms, int num_geoms);

struct GridShape {               // ptk::SceneTables::grid_*
  int res[3];
  float gmin[3], cs[3], inv_cs[3], pad;
};
struct Grid {
  GridShape shape{};
  size_t guard = 0;              // empty cells in front of and behind the cell table proper (build_scene_tables)
  std::vector<uint32_t> start;   // cell c's records: items[start[guard + c] .. start[guard + c + 1])
  std::vector<ptd::Node> items, items_b;  // items_b: centre / half extent copies, empty unless asked for
};
bool build_grid(const std::vector<ptd::Node>& nodes, const PtGeom* geoms, int num_geoms, const float root_min[3], const float root_max[3],
                double coord_mag, double density, bool forced, Grid& grid);
void origin_region(const float root_min[3], const float root_max[3], const float cam[3], double olo[3], double ohi[3]);
int tighten_sphere_leaves(std::vector<ptd::Node>& nodes, const PtGeom* geoms, const double origin_lo[3], const double origin_hi[3]);
double scene_magnitude(const float root_min[3], const float root_max[3], const float cam[3]);
void center_half_box(float bmin[3], float bmax[3], bool inner, double magnitude);  // magnitude: scene_magnitude(), used for inner boxes only

struct HostTables {              // what ptk::SceneTables points to, on the host
  std::vector<ptd::Node> nodes, nodes_b;  // *_b: centre / half extent copies (`center_half`), else empty
  std::vector<ptd::TopEntry> top, top_b;
  std::vector<ptd::Geom> geoms;
  std::vector<ptd::Mat> mats;
  std::vector<Grid> grids;       // candidates for choose_traversal, the cost model's resolution first
  unsigned long long top_xor = 0;
  float root_min[3], root_max[3], cull_margin;
  int tight_leaves = 0;
  bool has_triangles = false;
};
// debug_flags: PtOptions.debug_flags; center_half: ptk::KernelApi::boxes_center_half
HostTables build_scene_tables(const PtSceneDesc& desc, int debug_flags, bool center_half);

}  // namespace pt
