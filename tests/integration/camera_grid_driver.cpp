// The host twin of the device grid build, stand-alone: pt_tables.cpp and pt_scene.cpp are plain C++, so the system compiler builds them
// with this file under -fsanitize=address,undefined and tests/test_camera_grid_host.py runs the program directly.  The small grids of
// that test and 257 x 32 x 32 with the per_block population of tests/camera_grid_ref.py (1 + b % 3 tiny leaves in the first cell of
// every 1024-cell block b, one in the last cell, an inner node in front of two leaves of three), with and without the copies, and a
// whole-grid leaf on each: every vector is exactly as large as the build may touch, so an access past an end is reported.  The checks
// here are the cell table's invariants; the comparison with the restatement is the Python test's.  One line and exit status 0 when
// nothing was found.
#include <cstdio>
#include <vector>

#include "pt_tables.h"

static int run(const int res[3], bool whole, bool center_half, int* cases) {
  const int64_t ncell = (int64_t)res[0] * res[1] * res[2];
  const float root_min[3] = {0.f, 0.f, 0.f}, root_max[3] = {(float)res[0], (float)res[1], (float)res[2]};
  std::vector<ptd::Node> nodes;
  auto leaf = [&](const float lo[3], const float hi[3]) {
    if (nodes.size() % 3 != 1) {  // an inner node: the build skips it
      ptd::Node in{};
      for (int a = 0; a < 3; ++a) in.bmax[a] = root_max[a];
      in.geom = -1;
      nodes.push_back(in);
    }
    ptd::Node n{};
    for (int a = 0; a < 3; ++a) n.bmin[a] = lo[a], n.bmax[a] = hi[a];
    n.geom = (int32_t)nodes.size();  // (patched below to a valid geom)
    nodes.push_back(n);
  };
  auto tiny = [&](int64_t c) {
    const float x = (float)(c % res[0]) + 0.5f, y = (float)((c / res[0]) % res[1]) + 0.5f, z = (float)(c / ((int64_t)res[0] * res[1])) + 0.5f;
    const float lo[3] = {x - 0.01f, y - 0.01f, z - 0.01f}, hi[3] = {x + 0.01f, y + 0.01f, z + 0.01f};
    leaf(lo, hi);
  };
  if (whole) leaf(root_min, root_max);
  const int64_t blocks = (ncell + 1023) / 1024;
  for (int64_t b = 0; b < blocks; ++b)
    for (int k = 0; k < 1 + (int)(b % 3); ++k) tiny(b * 1024);
  tiny(ncell - 1);
  int leaves = 0;
  for (ptd::Node& n : nodes)
    if (n.geom >= 0) ++leaves;
  std::vector<int32_t> types((size_t)leaves);
  int next = 0;
  for (ptd::Node& n : nodes)
    if (n.geom >= 0) n.geom = leaves - 1 - next, types[(size_t)next] = next % 3, ++next;
  PtCameraGridResult out{};
  pt::Grid grid;
  pt::camera_grid_host(nodes.data(), (int)nodes.size(), types.data(), leaves, root_min, root_max, 0.0, res, center_half, &out, grid);
  if (out.status != 0) return 4;
  const size_t guard = out.guard, words = (size_t)ncell + 1 + 2 * guard;
  if (out.num_cells != ncell || grid.start.size() != words || grid.items.size() != out.refs) return 5;
  if (grid.items_b.size() != (center_half ? grid.items.size() : 0)) return 6;
  uint32_t longest = 0;
  for (size_t i = 0; i + 1 < words; ++i) {
    if (grid.start[i] > grid.start[i + 1]) return 7;
    longest = grid.start[i + 1] - grid.start[i] > longest ? grid.start[i + 1] - grid.start[i] : longest;
  }
  if (grid.start[guard] != 0 || grid.start[guard + (size_t)ncell] != out.refs || grid.start.back() != out.refs || longest != out.longest) return 8;
  const uint64_t want = (uint64_t)leaves - (whole ? 1 : 0) + (whole ? (uint64_t)ncell : 0);
  if (out.refs != want) return 9;
  for (size_t c = 0; c < (size_t)ncell; ++c)  // threaded order inside every cell
    for (uint32_t j = grid.start[guard + c] + 1; j < grid.start[guard + c + 1]; ++j)
      if (grid.items[j - 1].skip >= grid.items[j].skip) return 10;
  ++*cases;
  return 0;
}

int main() {
  const int grids[8][3] = {{1, 1, 1}, {33, 31, 1}, {32, 32, 1}, {41, 25, 1}, {512, 1, 1}, {1, 1, 512}, {3, 5, 7}, {257, 32, 32}};
  int cases = 0;
  for (const auto& g : grids)
    for (int whole = 0; whole < 2; ++whole)
      for (int center_half = 0; center_half < 2; ++center_half)
        if (const int rc = run(g, whole != 0, center_half != 0, &cases)) return rc;
  // beyond the limits nothing is built and nothing is left behind
  const int big[3] = {257, 128, 128};
  const float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {257.f, 128.f, 128.f};
  ptd::Node n{};
  for (int a = 0; a < 3; ++a) n.bmax[a] = hi[a];
  const int32_t type = 0;
  PtCameraGridResult out{};
  pt::Grid grid;
  pt::camera_grid_host(&n, 1, &type, 1, lo, hi, 0.0, big, false, &out, grid);
  if (out.status != PT_DEVICE_TABLES_CELLS || out.refs != 0 || !grid.start.empty() || !grid.items.empty()) return 11;
  std::printf("camera grid: %d cases\n", cases + 1);
  return 0;
}
