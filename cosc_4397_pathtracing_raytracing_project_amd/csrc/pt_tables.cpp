// pt_tables.cpp — the scene tables of the MI355X path tracer (pt_tables.h), pure host arithmetic.  Compiled with
// -ffp-contract=off like the kernels' exact build: box_normal_table must round as the device does.
#include "pt_tables.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "pt_camera_tables.h"
#include "pt_scene.h"

namespace pt {

// Re-emit the reference-order BVH (node, left, right links) in visiting order with
// skip links (see ptd::Node).  Visiting order of the reference's stack walk is:
// node, then its RIGHT subtree, then its LEFT subtree (pathtrace.cu:321-322).
static void thread_bvh(const std::vector<PtBVHNode>& in, int idx, std::vector<ptd::Node>& out, std::vector<int>& where) {
  const PtBVHNode& n = in[idx];
  const size_t self = out.size();
  where[idx] = (int)self;
  ptd::Node t{};
  std::memcpy(t.bmin, n.bmin, 12);
  std::memcpy(t.bmax, n.bmax, 12);
  t.geom = n.left < 0 ? n.geomIndex : -1;
  out.push_back(t);
  if (n.left >= 0) {
    thread_bvh(in, n.right, out, where);
    thread_bvh(in, n.left, out, where);
  }
  out[self].skip = (int32_t)out.size();
}
ThreadedBvh threaded_bvh(const PtGeom* geoms, int num_geoms) {
  ThreadedBvh t;
  pt::buildBVH(geoms, num_geoms, t.ref);
  t.nodes.reserve(t.ref.size());
  t.where.assign(t.ref.size(), -1);
  thread_bvh(t.ref, 0, t.nodes, t.where);
  return t;
}

// Flatten the top of the tree into at most ptd::kMaxTop entries (see ptd::TopEntry): start from
// the root and keep splitting the inner entry that covers the most nodes.  The entries are emitted in
// path-code order (0 = left child, 1 = right child, root choice in the most significant bit); when
// the cut is a complete level (every entry at the same depth, a power of two of them) `top_xor`
// receives, per direction-sign octant, the XOR mask that turns list order into near-first order
// (pt_kernels.hip permute_xor), otherwise 0.
static void build_top(const std::vector<PtBVHNode>& ref, const std::vector<ptd::Node>& thr, const std::vector<int>& where,
                      const PtGeom* geoms, std::vector<ptd::TopEntry>& top, unsigned long long* top_xor) {
  struct Cut {
    int ref_idx;
    uint32_t code;
    int len;
  };
  std::vector<Cut> cut{{0, 0u, 0}};
  auto span = [&](int ref_idx) { return thr[where[ref_idx]].skip - where[ref_idx]; };
  while ((int)cut.size() < ptd::kMaxTop) {
    int best = -1;
    for (size_t i = 0; i < cut.size(); ++i)
      if (ref[cut[i].ref_idx].left >= 0 && cut[i].len < 24 && (best < 0 || span(cut[i].ref_idx) > span(cut[best].ref_idx)))
        best = (int)i;
    if (best < 0) break;
    const Cut c = cut[best];
    const PtBVHNode n = ref[c.ref_idx];
    cut[best] = Cut{n.left, c.code << 1, c.len + 1};
    cut.push_back(Cut{n.right, (c.code << 1) | 1u, c.len + 1});
  }
  std::sort(cut.begin(), cut.end(), [](const Cut& a, const Cut& b) {
    return ((uint64_t)a.code << (32 - a.len)) < ((uint64_t)b.code << (32 - b.len));
  });
  top.clear();
  for (const Cut& c : cut) {
    const PtBVHNode& n = ref[c.ref_idx];
    ptd::TopEntry e{};
    std::memcpy(e.bmin, n.bmin, 12);
    std::memcpy(e.bmax, n.bmax, 12);
    e.idx = where[c.ref_idx];
    e.link = n.left < 0 ? -1 - geoms[n.geomIndex].type : thr[where[c.ref_idx]].skip;
    top.push_back(e);
  }
  *top_xor = 0;
  const int levels = cut[0].len;
  bool complete = levels >= 1 && levels <= 5 && (int)cut.size() == (1 << levels);
  for (const Cut& c : cut) complete = complete && c.len == levels;
  if (!complete) return;
  // axis and polarity of each level, taken from the node on the all-left path
  int axis[5] = {0, 0, 0, 0, 0};
  bool left_lower[5] = {true, true, true, true, true};
  int at = 0;
  for (int l = 0; l < levels; ++l) {
    const PtBVHNode &L = ref[ref[at].left], &R = ref[ref[at].right];
    float sep = -1.f;
    for (int a = 0; a < 3; ++a) {
      const float d = fabsf((L.bmin[a] + L.bmax[a]) - (R.bmin[a] + R.bmax[a]));
      if (d > sep) sep = d, axis[l] = a;
    }
    left_lower[l] = (L.bmin[axis[l]] + L.bmax[axis[l]]) <= (R.bmin[axis[l]] + R.bmax[axis[l]]);
    at = ref[at].left;
  }
  for (int oct = 0; oct < 8; ++oct) {
    uint32_t m = 0;
    for (int l = 0; l < levels; ++l) {
      const bool negative = (oct >> axis[l]) & 1;
      const bool near_is_right = left_lower[l] == negative;  // positive direction: the lower child is nearer
      if (near_is_right) m |= 1u << (levels - 1 - l);
    }
    *top_xor |= (unsigned long long)m << (8 * oct);
  }
}

// normalize(vec3(invTranspose * vec4(n, 0))) in GLM operation order (same expressions as mulMV /
// normalize in pt_kernels.hip; this file is compiled with -ffp-contract=off, sqrtf and / are IEEE on
// the host as on the device), for the 7 object-space normals a cube test can produce.
static void box_normal_table(const float invT12[12], float out[7][4]) {
  for (int code = 0; code < 7; ++code) {
    float n[3] = {0.f, 0.f, 0.f};
    if (code > 0) n[(code - 1) / 2] = ((code - 1) & 1) ? 1.0f : -1.0f;
    const float* m = invT12;
    float v[3];
    for (int r = 0; r < 3; ++r) v[r] = (m[0 + r] * n[0] + m[3 + r] * n[1]) + (m[6 + r] * n[2] + m[9 + r] * 0.0f);
    const float inv = 1.0f / sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    out[code][0] = v[0] * inv, out[code][1] = v[1] * inv, out[code][2] = v[2] * inv, out[code][3] = 0.f;
  }
}

static void pack_rows(const float m16[16], float out12[12]) {
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 3; ++r) out12[c * 3 + r] = m16[c * 4 + r];
}

// Tighter leaf boxes for spheres (large scenes only; result-neutral).  The reference's leaf box is the box of the
// transformed unit CUBE (pathtrace.cu:36-50), which for a rotated sphere / ellipsoid is up to sqrt(3) wider per axis than
// the primitive: rays pass the box, reach sphereIntersectionTest (intersections.h:102-144) and miss.  Our structures may
// skip such a leaf exactly when its primitive test cannot report a hit, so the box our traversal tests is
//     reference leaf box  INTERSECTED WITH  box of the ellipsoid { x : |A (x - c)| <= rho },  A = the geom's inverse transform,
// where rho > 0.5 covers everything the reference's float arithmetic can still call a hit.  That test takes
// radicand = v*v - (|ro|^2 - 0.25) >= 0 with ro = A o + t, rd = normalize(A d), v = ro . rd in float (u = 2^-24):
//   * the two dot products, the square and the two subtractions:  <= 18 u |ro|^2,         |ro| <= |A|_F * D  =: D_obj
//   * rounding of ro itself (4 products per component, cancelling against t when the object is far from the origin):
//     |d ro| <= 14 u (|A|_F * M + |t|) =: 14 u M_obj, which moves the squared distance to the axis by <= 2 * 0.5 * |d ro|
//   * rounding of rd (direction error <= 5 u cond(A)), which moves it by <= 5 u cond(A) * D_obj
// with D = the largest distance from a ray origin to the sphere's centre and M = the largest coordinate magnitude of a ray
// origin; ray origins of the renderer lie in the scene bounds (hit points) or at the camera.  rho^2 = 0.25 + 4 x that sum
// (safety factor 3.5 on the dominant term), the box is rounded outward and padded by 32 float-eps of M for the slab test's
// own rounding.  The tightened box lies inside the reference's, so a ray that passes it passes the reference's box and
// every ancestor (the slab test is monotone under inclusion, DESIGN.md §9, LABNOTES.md §9.1): the leaves we test are a subset of the
// reference's, and the ones we drop return "no hit" there.  Exact mode stays bit-identical (tests: stress scenes and the
// random-scene fuzz against the oracle, which keeps the reference's boxes); debug_flags 2048 keeps the reference's boxes.
// pt_stage_intersect on such a scene inherits the assumption about ray origins.
// One sphere: ptct::sphere_tight_box (pt_camera_tables.h), the arithmetic the device build of the tables runs as well.
int tighten_sphere_leaves(std::vector<ptd::Node>& nodes, const PtGeom* geoms, const double origin_lo[3], const double origin_hi[3]) {
  int tightened = 0;
  for (ptd::Node& n : nodes) {
    if (n.geom < 0 || geoms[n.geom].type != PT_GEOM_SPHERE) continue;
    float lo[3], hi[3];
    if (!ptct::sphere_tight_box(geoms[n.geom].inverseTransform, origin_lo, origin_hi, n.bmin, n.bmax, lo, hi)) continue;
    std::memcpy(n.bmin, lo, 12);
    std::memcpy(n.bmax, hi, 12);
    ++tightened;
  }
  return tightened;
}
// The region ray origins come from: hit points (inside the scene bounds; the shading offsets are <= 1e-3) and the camera.
void origin_region(const float root_min[3], const float root_max[3], const float cam[3], double olo[3], double ohi[3]) {
  for (int a = 0; a < 3; ++a) {
    const double ext = (double)root_max[a] - (double)root_min[a];
    olo[a] = std::min((double)root_min[a] - 0.01 * ext - 0.01, (double)cam[a]);
    ohi[a] = std::max((double)root_max[a] + 0.01 * ext + 0.01, (double)cam[a]);
  }
}

// Uniform grid over the leaf boxes — the traversal structure of our own for large scenes (SceneTables::grid_*).  The
// reference's median-split BVH (pathtrace.cu:52-111) costs a bounce ray of a 10 000-primitive scene ~60 dependent node
// fetches below the top list; a grid with about one cell per primitive is walked in ~6 cells.  Results cannot change: a
// leaf is tested exactly when the ray passes the leaf's own box (pt_device.h), the grid only has to deliver a superset
// of those leaves, and it does because every leaf is listed in all cells its box grown by `pad` touches — `pad` is orders
// of magnitude above the rounding of the float cell walk.  Built for large scenes whose lists stay moderate; whether
// the renderer walks it or the BVH is measured at init (choose_traversal).
// `coord_mag`: the largest coordinate magnitude a ray of this scene is built from (scene bounds and, where known, the
// camera position).  The float cell walk's error grows with eps * |coordinate| and eps * t_in, not with the extent, so
// for a small scene far from the origin (|coordinate| / extent >~ 1e3) 1e-4 * extent alone would sink below the
// walk's rounding; the pad therefore never goes below 64 ulps of that magnitude.
// The grid's frame for a scene's bounds: pad, lower corner and extent, or false where no grid is built (an empty or non-finite extent, a
// scene that is a speck at its distance from the origin).  Host arithmetic for both builds of the tables.
bool grid_frame(const float root_min[3], const float root_max[3], double coord_mag, ptct::GridFrame& f) {
  double maxext = 0.0;
  for (int a = 0; a < 3; ++a) maxext = std::max(maxext, (double)root_max[a] - (double)root_min[a]);
  if (!(maxext > 0.0) || !std::isfinite(maxext)) return false;
  for (int a = 0; a < 3; ++a) coord_mag = std::max({coord_mag, std::fabs((double)root_min[a]), std::fabs((double)root_max[a])});
  f.pad = std::max(1e-4 * maxext, 64.0 * (double)FLT_EPSILON * coord_mag);
  if (!(f.pad < 0.05 * maxext)) return false;  // the scene is a speck at its distance from the origin: cells would be all padding
  for (int a = 0; a < 3; ++a) {
    f.lo[a] = (double)root_min[a] - 2.0 * f.pad;
    f.ext[a] = ((double)root_max[a] + 2.0 * f.pad) - f.lo[a];
  }
  return true;
}
// The shape the kernels read, for the resolution in f.res; returns the number of cells.
int64_t grid_shape(const ptct::GridFrame& f, GridShape& s) {
  int64_t ncell = 1;
  for (int a = 0; a < 3; ++a) {
    s.res[a] = f.res[a];
    s.gmin[a] = (float)f.lo[a];
    s.cs[a] = (float)(f.ext[a] / s.res[a]);
    s.inv_cs[a] = (float)(s.res[a] / f.ext[a]);
    ncell *= s.res[a];
  }
  s.pad = (float)f.pad;
  return ncell;
}
size_t grid_guard(const GridShape& s) { return (size_t)s.res[0] * s.res[1] + s.res[0] + 2; }

// The scalars as camera_tables() and build_grid() compute them for a kFixed request, with build_grid's refusals that need no count
// and the device build's limit on the cells.
GridVerdict device_grid_scalars(const float root_min[3], const float root_max[3], double coord_mag, const int res[3], int64_t num_geoms,
                                ptct::GridFrame& frame, GridShape& shape, int64_t* ncell, size_t* guard) {
  *ncell = 0, *guard = 0;
  if (!grid_frame(root_min, root_max, coord_mag, frame)) return kGridNone;
  for (int k = 0; k < 3; ++k) frame.res[k] = std::min(512, std::max(1, res[k]));
  *ncell = grid_shape(frame, shape);
  *guard = grid_guard(shape);
  if (*ncell > (int64_t)64 * 1024 * 1024 || num_geoms > (1 << 24)) return kGridNone;  // build_grid's refusals
  if (*ncell > ptct::kDeviceMaxCells) return kGridCells;
  return kGridBuild;
}
// build_grid's refusals on what the kernels counted (no reference: no leaf, which a renderer's tree never is), then the device build's limits
GridVerdict device_grid_counted(bool forced, int64_t leaves, unsigned long long refs, uint32_t longest, size_t scratch_cap) {
  if (refs == 0 || (int64_t)refs > ptct::kMaxRefs || (!forced && (int64_t)refs > 64 * leaves) || (!forced && longest > 4096)) return kGridNone;
  if (longest > ptct::kDeviceMaxList || refs > scratch_cap) return kGridList;
  return kGridBuild;
}

bool build_grid(const std::vector<ptd::Node>& nodes, const PtGeom* geoms, int num_geoms, const float root_min[3], const float root_max[3],
                double coord_mag, double density, bool forced, Grid& grid, const int* fixed_res) {
  std::vector<int> leaves;
  for (size_t i = 0; i < nodes.size(); ++i)
    if (nodes[i].geom >= 0) leaves.push_back((int)i);
  if (leaves.empty()) return false;
  ptct::GridFrame frame;
  if (!grid_frame(root_min, root_max, coord_mag, frame)) return false;
  const double* ext = frame.ext;
  double vol = 1.0;
  for (int a = 0; a < 3; ++a) vol *= ext[a];
  // the cells [c0, c1] per axis that a leaf's box grown by `pad` touches, at resolution `res` (pt_camera_tables.h)
  auto cell_range = [&](const ptd::Node& n, const int res[3], int c0[3], int c1[3]) {
    ptct::GridFrame f = frame;
    std::memcpy(f.res, res, sizeof(f.res));
    ptct::cell_range(n.bmin, n.bmax, f, c0, c1);
  };
  auto references = [&](const int res[3]) {
    int64_t refs = 0;
    for (int li : leaves) {
      int c0[3], c1[3];
      cell_range(nodes[li], res, c0, c1);
      refs += (int64_t)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
    }
    return refs;
  };
  // Resolution: about one cell per primitive (density <= 0: a search around that).  What a ray pays is one step per cell
  // it crosses plus one box test per record it comes across, i.e. per unit length ~ r (cells) and ~ refs * r / ncell
  // (records), r = mean resolution; measured on the 10 170-primitive scene a record costs about half a step (kernel
  // time follows refs * r / ncell + 2 r over resolutions 15..31).  The search matters for primitives on a lattice —
  // the resolution that matches the lattice pitch halves the references — and is harmless otherwise.
  auto resolution = [&](double per_len, int res[3]) {
    for (int a = 0; a < 3; ++a) res[a] = (int)std::min(512.0, std::max(1.0, std::floor(ext[a] * per_len + 0.5)));
  };
  GridShape& s = grid.shape;
  const double base = std::cbrt((double)leaves.size() / vol);
  if (fixed_res) {
    for (int a = 0; a < 3; ++a) s.res[a] = std::min(512, std::max(1, fixed_res[a]));
  } else if (density > 0.0) {
    resolution(std::cbrt(density) * base, s.res);
  } else {
    double best_cost = INFINITY;
    int last[3] = {0, 0, 0};
    for (int i = 0; i <= 40; ++i) {
      int res[3];
      resolution(base * (0.6 + 0.025 * i), res);
      if (res[0] == last[0] && res[1] == last[1] && res[2] == last[2]) continue;
      std::memcpy(last, res, sizeof(last));
      const double r = (res[0] + res[1] + res[2]) / 3.0, cells = (double)res[0] * res[1] * res[2];
      const double cost = (double)references(res) * r / cells + 2.0 * r;
      if (cost < best_cost) best_cost = cost, std::memcpy(s.res, res, sizeof(res));
    }
  }
  std::memcpy(frame.res, s.res, sizeof(frame.res));
  const int64_t ncell = grid_shape(frame, s);
  if (ncell > (int64_t)64 * 1024 * 1024) return false;
  const int64_t refs = references(s.res);
  if (refs > ptct::kMaxRefs) return false;  // ring entries hold 22-bit record indices
  if (num_geoms > (1 << 24)) return false;    // records hold 24-bit geom indices
  // a candidate only while the lists stay moderate (whether it beats the BVH scan is measured, choose_traversal())
  if (!forced && refs > 64 * (int64_t)leaves.size()) return false;
  auto cell = [&](int x, int y, int z) { return (size_t)x + (size_t)s.res[0] * ((size_t)y + (size_t)s.res[1] * z); };
  std::vector<uint32_t> count((size_t)ncell + 1, 0);
  for (int li : leaves) {
    int c0[3], c1[3];
    cell_range(nodes[li], s.res, c0, c1);
    for (int z = c0[2]; z <= c1[2]; ++z)
      for (int y = c0[1]; y <= c1[1]; ++y)
        for (int x = c0[0]; x <= c1[0]; ++x) ++count[cell(x, y, z)];
  }
  uint32_t longest = 0;
  grid.start.assign((size_t)ncell + 1, 0);
  for (int64_t c = 0; c < ncell; ++c) {
    grid.start[c + 1] = grid.start[c] + count[c];
    longest = std::max(longest, count[c]);
  }
  if (!forced && longest > 4096) return false;
  grid.items.assign((size_t)refs, ptd::Node{});
  std::vector<uint32_t> fill(grid.start.begin(), grid.start.end() - 1);
  for (int li : leaves) {  // threaded (= reference visiting) order inside every cell
    int c0[3], c1[3];
    cell_range(nodes[li], s.res, c0, c1);
    for (int z = c0[2]; z <= c1[2]; ++z)
      for (int y = c0[1]; y <= c1[1]; ++y)
        for (int x = c0[0]; x <= c1[0]; ++x) {
          ptd::Node it = nodes[li];
          it.skip = li;
          it.geom = ptct::record_geom_word(x, y, z, c0, c1, geoms[nodes[li].geom].type, nodes[li].geom);
          grid.items[fill[cell(x, y, z)]++] = it;
        }
  }
  return true;
}

// A box as centre and half extent for the fast build's slab test (pt_arith.inc slab_t): the centre rounded to float, the half
// extent rounded UP from the distance to the farther face (so the converted box contains the original in real arithmetic), in
// place in (bmin, bmax).  `inner` (inner nodes, subtree entries of the top list — pure acceleration): a little more, so that in the
// test's float arithmetic a ray that passes a leaf's box still passes every box above it.  How much more, with u = 2^-24, i the
// reciprocal direction and n = -o * i of the ray (both computed once per ray: the same values for the leaf and its ancestor),
// per plane and per box:
//   * tc = fma(c, i, n) is off by <= u |tc| <= u (|c| + |o|) |i|, the plane fma(-+h, |i|, tc) by <= u (|c| + |o| + h) |i| more;
//   * the converted LEAF reaches <= 2 u (|c| + h) beyond its min / max box (centre rounded, half extent rounded up), and only
//     that min / max box is known to lie inside the ancestor's.
// Leaf plus ancestor: <= (4 (|o| + |c| + h) + 2 (|c| + h)) u |i| <= 10 u M |i| for |o|, |c| + h <= M.  The error follows the ray
// ORIGIN, not the box: a small node next to the world origin of a wide scene needs the margin of the whole scene.  So the slack is
// 1e-5 of the half extent plus 1e-5 * `magnitude`, M = scene_magnitude() (where ray origins lie: the scene bounds, the camera):
// 1e-5 / (10 u) = 16.7 times the bound.
void center_half_box(float bmin[3], float bmax[3], bool inner, double magnitude) { ptct::center_half_box(bmin, bmax, inner, magnitude); }
// The largest coordinate magnitude a ray origin of the scene has: hit points lie in the scene bounds, depth 0 starts at the camera.
double scene_magnitude(const float root_min[3], const float root_max[3], const float cam[3]) {
  double m = 0.0;
  for (int a = 0; a < 3; ++a) m = std::max({m, std::fabs((double)root_min[a]), std::fabs((double)root_max[a]), std::fabs((double)cam[a])});
  return m;
}

// What a renderer's grid has beyond build_grid's: the guard cells and, for the fast build, the copies of the records.
static void renderer_grid(Grid& grid, bool center_half) {
  // the cell table with empty cells before and after it: a walk may run up to one cell per axis past the grid's far side
  // before its distance test ends it (pt_grid.inc CellWalk)
  grid.guard = grid_guard(grid.shape);
  const uint32_t total = grid.start.back();
  grid.start.insert(grid.start.begin(), grid.guard, 0u);
  grid.start.resize(grid.start.size() + grid.guard, total);
  if (center_half) {  // the grid's records are leaf boxes
    grid.items_b = grid.items;
    for (ptd::Node& n : grid.items_b) center_half_box(n.bmin, n.bmax, false, 0.0);
  }
}

// What follows the camera position (pt_tables.h).  The order matters: the copies and the grids are made from the tightened boxes.
void camera_tables(HostTables& t, const CameraBase& base, const float cam[3], int debug_flags, bool center_half, const GridRequest& request) {
  t.nodes = base.nodes;
  t.top = base.top;
  t.tight_leaves = 0;
  if ((int)t.nodes.size() >= kTightNodes && !(debug_flags & 2048)) {
    double olo[3], ohi[3];
    origin_region(t.root_min, t.root_max, cam, olo, ohi);
    t.tight_leaves = tighten_sphere_leaves(t.nodes, base.geoms.data(), olo, ohi);
    for (ptd::TopEntry& e : t.top)
      if (e.link < 0) std::memcpy(e.bmin, t.nodes[e.idx].bmin, 12), std::memcpy(e.bmax, t.nodes[e.idx].bmax, 12);
  }
  {
    // SceneTables::cull_margin: >= 10x the worst undershoot of a reported hit distance (1e-4 object units mapped
    // to world space + rounding of the transforms at the scene's coordinate magnitudes)
    const float extent = std::max(1.0f, (float)scene_magnitude(t.root_min, t.root_max, cam));
    t.cull_margin = 1e-3f * base.max_xf + 1e-4f * extent;
  }
  t.nodes_b.clear(), t.top_b.clear();
  if (center_half) {  // the fast build: converted copies for the bounce kernels
    const double mag = scene_magnitude(t.root_min, t.root_max, cam);
    t.nodes_b = t.nodes;
    for (ptd::Node& n : t.nodes_b) center_half_box(n.bmin, n.bmax, n.geom < 0, mag);
    t.top_b = t.top;
    for (ptd::TopEntry& e : t.top_b) center_half_box(e.bmin, e.bmax, e.link >= 0, mag);
  }
  t.grids.clear();
  const bool forced = (debug_flags & 256) != 0;
  const bool candidates = request.kind == GridRequest::kCandidates && ((int)t.nodes.size() >= kGridNodes || forced);
  if ((candidates || request.kind == GridRequest::kFixed) && !(debug_flags & 512)) {
    double cam_mag = 0.0;
    for (int a = 0; a < 3; ++a) cam_mag = std::max(cam_mag, std::fabs((double)cam[a]));
    // Candidates: the resolution the host's cost model finds (about one cell per primitive; build_grid) and two finer ones.
    // The model prices a uniform spread of primitives and rays; where the primitives cluster, a finer grid pays (clustered 1500
    // objects: 2319 Msamples/s at the model's resolution, 2931 at 8 cells per primitive; a lattice wants exactly its pitch),
    // so choose_traversal() measures.  A forced grid (debug_flags 256) is the only candidate, as is one of a given resolution.
    std::vector<double> densities{0.0};
    if (!forced && candidates) densities.insert(densities.end(), {4.0, 8.0});
    for (double density : densities) {
      Grid grid;
      if (!build_grid(t.nodes, base.geoms.data(), (int)base.geoms.size(), t.root_min, t.root_max, cam_mag, density, forced, grid,
                      candidates ? nullptr : request.res))
        continue;
      bool repeat = false;
      for (const Grid& o : t.grids) repeat = repeat || std::equal(o.shape.res, o.shape.res + 3, grid.shape.res);
      if (repeat) continue;
      renderer_grid(grid, center_half);
      t.grids.push_back(std::move(grid));
    }
  }
}

std::vector<ptd::Mat> material_table(const PtMaterial* materials, int num_materials) {
  std::vector<ptd::Mat> mats((size_t)std::max(num_materials, 0), ptd::Mat{});
  for (int i = 0; i < num_materials; ++i) {
    const PtMaterial& m = materials[i];
    std::memcpy(mats[i].color, m.color, 12);
    std::memcpy(mats[i].spec, m.specular_color, 12);
    mats[i].reflective = m.hasReflective, mats[i].refractive = m.hasRefractive, mats[i].emittance = m.emittance;
  }
  return mats;
}

HostTables build_scene_tables(const PtSceneDesc& desc, int debug_flags, bool center_half, const GridRequest& request, CameraBase* keep) {
  HostTables t;
  CameraBase base;
  ThreadedBvh bvh = threaded_bvh(desc.geoms, desc.num_geoms);
  build_top(bvh.ref, bvh.nodes, bvh.where, desc.geoms, base.top, &t.top_xor);
  base.nodes = std::move(bvh.nodes);
  base.geoms.assign(desc.geoms, desc.geoms + desc.num_geoms);
  std::memcpy(t.root_min, bvh.ref[0].bmin, 12);
  std::memcpy(t.root_max, bvh.ref[0].bmax, 12);
  for (int i = 0; i < desc.num_geoms; ++i) {
    const PtGeom& gm = desc.geoms[i];
    if (gm.type == PT_GEOM_TRIANGLE) continue;  // world-space test: the pull-back is 1e-4 world units (max_xf >= 1 covers it)
    float f = 0.f;
    for (int c = 0; c < 3; ++c)
      for (int r = 0; r < 3; ++r) f += gm.transform[c * 4 + r] * gm.transform[c * 4 + r];
    base.max_xf = std::max(base.max_xf, sqrtf(f));
  }
  t.geoms.assign(desc.num_geoms, ptd::Geom{});
  for (int i = 0; i < desc.num_geoms; ++i) {
    const PtGeom& gm = desc.geoms[i];
    ptd::Geom& dg = t.geoms[i];
    dg.type = gm.type;
    dg.material = gm.materialid;
    if (gm.type == PT_GEOM_TRIANGLE) {  // mesh extension: the three world-space vertices where `inv` would be
      std::memcpy(dg.inv, gm.transform, 9 * sizeof(float));
      t.has_triangles = true;
      continue;
    }
    pack_rows(gm.inverseTransform, dg.inv);
    pack_rows(gm.transform, dg.xf);
    pack_rows(gm.invTranspose, dg.invT);
    box_normal_table(dg.invT, dg.box_normal);
  }
  t.mats = material_table(desc.materials, desc.num_materials);
  camera_tables(t, base, desc.camera.position, debug_flags, center_half, request);
  if (keep) *keep = std::move(base);
  return t;
}

GridRequest first_grid_request(const HostTables& t) {
  GridRequest r;
  r.kind = t.grids.empty() ? GridRequest::kNone : GridRequest::kFixed;
  if (!t.grids.empty()) std::memcpy(r.res, t.grids[0].shape.res, sizeof(r.res));
  return r;
}

// Bit i of the result: table i of the list in pt_amd.h (pt_camera_tables_host) differs between a and b.
template <typename T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static int tables_differ(const HostTables& a, const HostTables& b) {
  int d = 0;
  d |= same_bytes(a.nodes, b.nodes) ? 0 : 1;
  d |= same_bytes(a.nodes_b, b.nodes_b) ? 0 : 2;
  d |= same_bytes(a.top, b.top) ? 0 : 4;
  d |= same_bytes(a.top_b, b.top_b) ? 0 : 8;
  d |= same_bytes(a.geoms, b.geoms) ? 0 : 16;
  d |= same_bytes(a.mats, b.mats) ? 0 : 32;
  d |= std::memcmp(&a.cull_margin, &b.cull_margin, sizeof(float)) == 0 ? 0 : 64;
  d |= a.tight_leaves == b.tight_leaves && a.top_xor == b.top_xor ? 0 : 2048;
  if (a.grids.empty() != b.grids.empty()) return d | 128;
  if (a.grids.empty()) return d;
  const Grid &ga = a.grids[0], &gb = b.grids[0];
  d |= std::memcmp(&ga.shape, &gb.shape, sizeof(GridShape)) == 0 && ga.guard == gb.guard ? 0 : 128;
  d |= same_bytes(ga.start, gb.start) ? 0 : 256;
  d |= same_bytes(ga.items, gb.items) ? 0 : 512;
  d |= same_bytes(ga.items_b, gb.items_b) ? 0 : 1024;
  return d;
}

int camera_tables_check(const PtSceneDesc& desc, const PtCamera& cam, int debug_flags, bool center_half, int32_t grid_res_out[3], int32_t* tight_leaves,
                        int32_t* differing) {
  CameraBase base;
  const HostTables init = build_scene_tables(desc, debug_flags, center_half, GridRequest{}, &base);
  const GridRequest request = first_grid_request(init);
  HostTables moved = init;
  if (moved.grids.size() > 1) moved.grids.resize(1);
  const HostTables home = moved;
  camera_tables(moved, base, cam.position, debug_flags, center_half, request);
  PtSceneDesc there = desc;
  there.camera = cam;
  const HostTables fresh = build_scene_tables(there, debug_flags, center_half, request);
  int d = tables_differ(moved, fresh);
  camera_tables(moved, base, desc.camera.position, debug_flags, center_half, request);  // and back: what init built, at init's resolution
  d |= tables_differ(moved, home) << 16;
  for (int a = 0; a < 3; ++a) grid_res_out[a] = fresh.grids.empty() ? 0 : fresh.grids[0].shape.res[a];
  *tight_leaves = fresh.tight_leaves;
  *differing = d;
  return 0;
}

// ---- pt_camera_grid_host / pt_stage_camera_grid --------------------------------------------------------------------------------------
static_assert(sizeof(PtTableNode) == sizeof(ptd::Node) && sizeof(PtCameraGridResult) == 80, "the grid stage's records");
const char* camera_grid_refusal(const PtTableNode* nodes, int num_nodes, const int32_t* geom_types, int num_geoms, const float* root_min, const float* root_max,
                                double coord_mag, const int32_t* res, const PtCameraGridResult* out) {
  if (!nodes || !geom_types || !root_min || !root_max || !res || !out) return "null argument";
  if (num_nodes < 1 || num_geoms < 1) return "no nodes or no geoms";
  if (!(coord_mag >= 0.0) || !std::isfinite(coord_mag)) return "coord_mag is negative or not finite";
  for (int i = 0; i < num_nodes; ++i) {
    if (nodes[i].geom < -1 || nodes[i].geom >= num_geoms) return "a node's geom is outside [-1, num_geoms)";
    // (the host's reference count and the kernels' per-axis clamp agree only on boxes that are boxes)
    for (int a = 0; a < 3; ++a)
      if (!(nodes[i].bmin[a] <= nodes[i].bmax[a])) return "a node's box has bmin > bmax or a NaN";
  }
  return nullptr;
}
void camera_grid_result(const GridShape& s, size_t guard, int64_t ncell, unsigned long long refs, uint32_t longest, GridVerdict status, PtCameraGridResult* out) {
  std::memset(out, 0, sizeof(*out));
  for (int a = 0; a < 3; ++a) out->res[a] = s.res[a], out->origin[a] = s.gmin[a], out->cell_size[a] = s.cs[a], out->inv_cell_size[a] = s.inv_cs[a];
  out->pad = s.pad;
  out->guard = (uint32_t)guard, out->num_cells = ncell, out->refs = refs, out->longest = longest, out->status = (int32_t)status;
}
void camera_grid_host(const ptd::Node* nodes, int num_nodes, const int32_t* geom_types, int num_geoms, const float root_min[3], const float root_max[3],
                      double coord_mag, const int32_t res[3], bool center_half, PtCameraGridResult* out, Grid& grid) {
  grid = Grid{};
  ptct::GridFrame frame{};
  GridShape shape{};
  int64_t ncell = 0;
  size_t guard = 0;
  const int want[3] = {res[0], res[1], res[2]};
  GridVerdict v = device_grid_scalars(root_min, root_max, coord_mag, want, num_geoms, frame, shape, &ncell, &guard);
  unsigned long long refs = 0;
  uint32_t longest = 0;
  if (v == kGridBuild) {  // what k_ct_refs adds up, whether or not a grid follows
    int64_t leaves = 0;
    for (int i = 0; i < num_nodes; ++i) {
      if (nodes[i].geom < 0) continue;
      int c0[3], c1[3];
      ptct::cell_range(nodes[i].bmin, nodes[i].bmax, frame, c0, c1);
      refs += (unsigned long long)ptct::cell_references(c0, c1);
      ++leaves;
    }
    bool built = false;
    if (refs <= (unsigned long long)ptct::kMaxRefs) {  // (beyond it build_grid refuses, and the kernels count nothing: longest stays 0)
      std::vector<PtGeom> geoms((size_t)num_geoms, PtGeom{});
      for (int i = 0; i < num_geoms; ++i) geoms[(size_t)i].type = geom_types[i];
      const std::vector<ptd::Node> list(nodes, nodes + num_nodes);
      built = build_grid(list, geoms.data(), num_geoms, root_min, root_max, coord_mag, 0.0, true, grid, want);
      if (built)
        for (size_t c = 0; c + 1 < grid.start.size(); ++c) longest = std::max(longest, grid.start[c + 1] - grid.start[c]);
    }
    v = device_grid_counted(true, leaves, refs, longest, (size_t)ptct::kMaxRefs);
    if (v == kGridBuild && !built) v = kGridNone;
    if (v == kGridBuild) renderer_grid(grid, center_half);
    else grid = Grid{};
  }
  camera_grid_result(shape, guard, ncell, refs, longest, v, out);
}

}  // namespace pt
