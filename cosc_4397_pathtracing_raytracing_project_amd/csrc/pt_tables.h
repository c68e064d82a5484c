// pt_tables.h — the scene tables the renderer uploads, built on the host from a PtSceneDesc.  Plain C++, no HIP:
// pt_api.cpp uploads them, and its host-only helpers pt_traversal_boxes / pt_build_grid call the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/pt_amd.h"
#include "pt_camera_tables.h"
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
// fixed_res: a resolution taken as given (a renderer that moves its camera keeps the one chosen at init); the cost-model search and
// `density` are skipped, everything else (pad, refusals, records) is computed as for any grid
bool build_grid(const std::vector<ptd::Node>& nodes, const PtGeom* geoms, int num_geoms, const float root_min[3], const float root_max[3],
                double coord_mag, double density, bool forced, Grid& grid, const int* fixed_res = nullptr);
// The host scalars of a grid, for both builds of the camera-dependent tables (pt_camera_tables.h): the frame (false: no grid for these
// bounds and this coordinate magnitude), the shape for frame.res with the number of cells, the guard cells of a renderer's cell table.
bool grid_frame(const float root_min[3], const float root_max[3], double coord_mag, ptct::GridFrame& frame);
int64_t grid_shape(const ptct::GridFrame& frame, GridShape& shape);
size_t grid_guard(const GridShape& shape);
// What the device build of a kFixed grid decides on the host (pt_api.cpp move_tables_device, pt_stage.cpp pt_stage_camera_grid), and the
// host twin of that stage with it (camera_grid_host): build_grid's refusals (kGridNone) and the device build's own limits.
enum GridVerdict { kGridBuild = 0, kGridList = PT_DEVICE_TABLES_LIST, kGridCells = PT_DEVICE_TABLES_CELLS, kGridNone = PT_CAMERA_GRID_NONE };
// Before anything is counted: the frame for these bounds with `res` clamped to [1, 512], its shape, cells and guard cells.
GridVerdict device_grid_scalars(const float root_min[3], const float root_max[3], double coord_mag, const int res[3], int64_t num_geoms,
                                ptct::GridFrame& frame, GridShape& shape, int64_t* ncell, size_t* guard);
// On what the kernels counted.  leaves: as build_grid counts them for its 64-per-leaf rule; scratch_cap: the references the workspace holds.
GridVerdict device_grid_counted(bool forced, int64_t leaves, unsigned long long refs, uint32_t longest, size_t scratch_cap);
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
// The part of the tables that does not follow the camera and that the part that does is rebuilt from: a renderer keeps it from init
// (pt_ctx_set_camera), a few MB for 10 000 primitives.
struct CameraBase {
  std::vector<ptd::Node> nodes;    // the threaded BVH before tighten_sphere_leaves
  std::vector<ptd::TopEntry> top;  // the top list before it copies the tightened leaves
  std::vector<PtGeom> geoms;       // what sphere_tight_box and build_grid read
  float max_xf = 1.0f;             // cull_margin's share of the transforms
};
// Which grids camera_tables() builds: the candidates for choose_traversal(), one grid of a given resolution, or none.
struct GridRequest {
  enum Kind { kCandidates, kFixed, kNone } kind = kCandidates;
  int res[3] = {0, 0, 0};
};
// Everything in `t` that follows the camera position, from `base` and t.root_min / root_max: the tightened leaves in nodes and top,
// tight_leaves, cull_margin, the centre / half extent copies, the grids.  build_scene_tables() ends with it, and a renderer that
// moves its camera runs it again.  A kFixed grid that build_grid refuses for this camera leaves t.grids empty.
void camera_tables(HostTables& t, const CameraBase& base, const float cam[3], int debug_flags, bool center_half, const GridRequest& request);
// debug_flags: PtOptions.debug_flags; center_half: ptk::KernelApi::boxes_center_half; keep: receives the CameraBase
HostTables build_scene_tables(const PtSceneDesc& desc, int debug_flags, bool center_half, const GridRequest& request = GridRequest{},
                              CameraBase* keep = nullptr);
// The material table (ptd::Mat: the nine words the kernels read of a PtMaterial): build_scene_tables' for pt_init, and what
// pt_ctx_set_materials uploads into the table a live renderer has.
std::vector<ptd::Mat> material_table(const PtMaterial* materials, int num_materials);
// The grid a renderer without a timing probe has in use after build_scene_tables(): the cost model's candidate, as a request.
GridRequest first_grid_request(const HostTables& t);
// pt_camera_tables_host (include/pt_amd.h).
int camera_tables_check(const PtSceneDesc& desc, const PtCamera& cam, int debug_flags, bool center_half, int32_t grid_res_out[3], int32_t* tight_leaves,
                        int32_t* differing);
// pt_camera_grid_host and pt_stage_camera_grid (include/pt_amd.h).  What both refuse about their inputs: nullptr, or the reason.
const char* camera_grid_refusal(const PtTableNode* nodes, int num_nodes, const int32_t* geom_types, int num_geoms, const float* root_min, const float* root_max,
                                double coord_mag, const int32_t* res, const PtCameraGridResult* out);
void camera_grid_result(const GridShape& shape, size_t guard, int64_t ncell, unsigned long long refs, uint32_t longest, GridVerdict status, PtCameraGridResult* out);
// The host twin: *out as the stage fills it, and with status kGridBuild `grid` (guard cells in, items_b with center_half).
void camera_grid_host(const ptd::Node* nodes, int num_nodes, const int32_t* geom_types, int num_geoms, const float root_min[3], const float root_max[3],
                      double coord_mag, const int32_t res[3], bool center_half, PtCameraGridResult* out, Grid& grid);

}  // namespace pt
