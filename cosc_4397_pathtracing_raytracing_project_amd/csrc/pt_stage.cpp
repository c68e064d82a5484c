// pt_stage.cpp — the stage entry points (pt_stage_*) of the tests: single kernels of the pipeline on caller-supplied host arrays.
// They act on the default context (pt_context.h) and keep nothing: every device buffer is scratch, freed on return.  The C ABI of
// the stages takes plain SoA float arrays ([3][n]); the kernels stream three planes of 16-byte path records (ptd::PathBuf), so the
// stage wrappers pack / unpack on the host.
#include <cstring>

#include "pt_camera_tables_device.h"
#include "pt_context.h"
#include "pt_denoise.h"
#include "pt_history.h"
#include "pt_scene.h"

using namespace ptc;

namespace {
// A scratch device copy of host[0 .. n): *out, or the refusal under the stage's name.
template <typename T>
int device_copy(Scratch& sc, const char* who, const T* host, size_t n, T** out) {
  if (!(*out = sc.get<T>(n))) return pt_fail("%s: out of device memory", who);
  HIP_OK(hipMemcpy(*out, host, n * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}
// Scratch hit records for `cap` paths; false when the device has no room.
bool scratch_hits(Scratch& sc, size_t cap, ptd::HitBuf* hb) {
  hb->stride = cap;
  hb->t = sc.get<float>(cap);
  hb->n = sc.get<float>(3 * cap);
  hb->mat = sc.get<int32_t>(cap);
  hb->p = sc.get<float>(3 * cap);
  return hb->t && hb->n && hb->mat && hb->p;
}

struct StagePaths {
  ptd::PathBuf pb{};
  std::vector<ptd::Word4> host;
  size_t cap = 0;
  bool alloc(Scratch& sc, size_t cap_) {
    cap = cap_;
    pb.stride = (int64_t)cap;
    pb.r = sc.get<ptd::Word4>(3 * cap);
    host.assign(3 * cap, ptd::Word4{0.f, 0.f, 0.f, 0.f});
    return pb.r != nullptr;
  }
  void pack(int n, const float* o, const float* d, const float* c) {  // arrays are [3][n]; null = zeros
    for (int i = 0; i < n; ++i) {
      auto at = [&](const float* a, int k) { return a ? a[(size_t)k * n + i] : 0.0f; };
      host[i] = ptd::Word4{at(o, 0), at(o, 1), at(o, 2), at(d, 0)};
      host[cap + i] = ptd::Word4{at(d, 1), at(d, 2), at(c, 0), at(c, 1)};
      reinterpret_cast<float*>(&host[2 * cap])[(size_t)i * (ptd::kPathPlane2Bytes / 4)] = at(c, 2);
    }
  }
  int upload() { return hipMemcpy(pb.r, host.data(), host.size() * sizeof(ptd::Word4), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1; }
  int download() { return hipMemcpy(host.data(), pb.r, host.size() * sizeof(ptd::Word4), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1; }
  void unpack(int n, float* o, float* d, float* c) const {
    for (int i = 0; i < n; ++i) {
      const ptd::Word4 &w0 = host[i], &w1 = host[cap + i];
      const float cz = reinterpret_cast<const float*>(&host[2 * cap])[(size_t)i * (ptd::kPathPlane2Bytes / 4)];
      if (o) o[i] = w0.x, o[(size_t)n + i] = w0.y, o[2 * (size_t)n + i] = w0.z;
      if (d) d[i] = w0.w, d[(size_t)n + i] = w1.x, d[2 * (size_t)n + i] = w1.y;
      if (c) c[i] = w1.z, c[(size_t)n + i] = w1.w, c[2 * (size_t)n + i] = cz;
    }
  }
};

// What the two filter stages share: the frame and its feature planes (and the noise planes of the guided form) up, `launch` with
// the device arrays and a workspace, the filtered frame down.
template <typename Launch>
int filter_stage(Ctx& g, const char* who, size_t n, const float* rgb_sum, const float* planes, const float* noise_planes, float* rgb_avg, Launch launch) {
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  float *d_img = nullptr, *d_planes = nullptr, *d_noise = nullptr;
  char* d_ws = sc.get<char>(pt_denoise_workspace_bytes(n));
  if (!d_ws) return pt_fail("%s: out of device memory", who);
  if (device_copy(sc, who, rgb_sum, 3 * n, &d_img) || device_copy(sc, who, planes, 4 * PT_FEATURE_PLANES * n, &d_planes)) return -1;
  if (noise_planes && device_copy(sc, who, noise_planes, 4 * PT_NOISE_PLANES * n, &d_noise)) return -1;
  const float* d_out = nullptr;
  if (launch(d_img, d_planes, d_noise, d_ws, &d_out)) return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  HIP_OK(hipMemcpy(rgb_avg, d_out, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// What the two intersect stages share.  tight_rule: with tightened leaves, refuse origins outside the region the boxes were sized for.
template <typename Launch>
int intersect_stage(Ctx& g, const char* who, bool tight_rule, int n, const float* origin, const float* dir, float* t, float* normal,
                    int32_t* material, float* point, Launch launch) {
  if (tight_rule && g.tight_leaves > 0) {
    // the tightened sphere boxes of a large scene are sized for ray origins inside the scene bounds or at the camera
    // (sphere_tight_box): rays from elsewhere could lose grazing hits, so they are refused rather than traced differently
    double olo[3], ohi[3];
    pt::origin_region(g.scene.root_min, g.scene.root_max, g.cam.position, olo, ohi);
    for (int i = 0; i < n; ++i)
      for (int a = 0; a < 3; ++a) {
        const float v = origin[(size_t)a * n + i];
        if (!(v >= olo[a] && v <= ohi[a]))
          return pt_fail("%s: ray %d starts outside the scene bounds (this scene's sphere leaves are tightened for origins inside them; "
                      "PtOptions.debug_flags 2048 keeps the reference's boxes)", who, i);
      }
  }
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  ptd::Queues qs = single_queue(g, n);
  const size_t cap = qs.cap;
  StagePaths sp;
  const bool have_paths = sp.alloc(sc, cap);
  ptd::HitBuf hb{};
  int32_t* cnt = sc.get<int32_t>(16);
  if (!have_paths || !scratch_hits(sc, cap, &hb) || !cnt) return pt_fail("%s: out of device memory", who);
  sp.pack(n, origin, dir, nullptr);
  if (sp.upload()) return pt_fail("%s: upload failed", who);
  HIP_OK(hipMemcpy(cnt, &n, 4, hipMemcpyHostToDevice));
  launch(qs, cnt, sp.pb, hb);
  HIP_OK(hipStreamSynchronize(g.stream));
  HIP_OK(hipMemcpy(t, hb.t, (size_t)n * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(material, hb.mat, (size_t)n * 4, hipMemcpyDeviceToHost));
  for (int c = 0; c < 3; ++c) {
    HIP_OK(hipMemcpy(normal + (size_t)c * n, hb.n + c * cap, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(point + (size_t)c * n, hb.p + c * cap, (size_t)n * 4, hipMemcpyDeviceToHost));
  }
  return 0;
}
// The grid the fused kernels of `g` walk, or nullptr (PtStats.grid_cells == 0)
const Ctx::DeviceGrid* walked_grid(const Ctx& g) { return tables(g).use_grid && g.fuse_bounces ? &g.grids[g.grid_pick] : nullptr; }
}  // namespace

extern "C" {

int pt_stage_generate(int pix_begin, int n, float* origin, float* dir) {
  if (need(default_context(), "pt_stage_generate")) return -1;
  Ctx& g = *default_context();
  if (n <= 0) return 0;
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  ptd::Queues qs = single_queue(g, n);
  StagePaths sp;
  int32_t* cnt = sc.get<int32_t>(16);
  if (!sp.alloc(sc, (size_t)qs.cap) || !cnt) return pt_fail("pt_stage_generate: out of device memory");
  ptk::BatchInfo b{};
  b.iter_first = 1, b.K = 1, b.N = n, b.pixel_begin = pix_begin, b.trace_depth = g.depth;
  b.slot_shift = 30;
  b.aa_jitter = g.aa_jitter ? 1 : 0;
  g.k->generate(g.stream, g.grid, g.dcam, b, qs, sp.pb, cnt);
  HIP_OK(hipStreamSynchronize(g.stream));
  if (sp.download()) return pt_fail("pt_stage_generate: download failed");
  sp.unpack(n, origin, dir, nullptr);
  return 0;
}

int pt_stage_intersect(int n, const float* origin, const float* dir, float* t, float* normal, int32_t* material,
                       float* point) {
  if (need(default_context(), "pt_stage_intersect")) return -1;
  Ctx& g = *default_context();
  if (n <= 0) return 0;
  return intersect_stage(g, "pt_stage_intersect", true, n, origin, dir, t, normal, material, point, [&](const ptd::Queues& qs, const int32_t* cnt, ptd::PathBuf pb, ptd::HitBuf hb) {
    g.k->intersect(g.stream, g.grid, tables(g), qs, cnt, pb, hb, g.legacy, false);
  });
}

// The grid walk of the fused kernels (k_intersect_grid) on caller-supplied rays: pt_stage_intersect's arrays and miss convention.
// primary_form 1: as k_primary walks (the reference's arithmetic and boxes, any origin), 0: as k_paths walks (the mode's arithmetic,
// the bounce tables; with tightened leaves the origins pt_stage_intersect accepts).
int pt_stage_intersect_grid(int n, const float* origin, const float* dir, int primary_form, float* t, float* normal, int32_t* material,
                            float* point) {
  if (need(default_context(), "pt_stage_intersect_grid")) return -1;
  Ctx& g = *default_context();
  if (n <= 0) return 0;
  if (!walked_grid(g)) return pt_fail("pt_stage_intersect_grid: this context walks no grid (PtStats.grid_cells is 0; PtOptions.debug_flags 256 forces one)");
  if (!origin || !dir || !t || !normal || !material || !point) return pt_fail("pt_stage_intersect_grid: null argument");
  return intersect_stage(g, "pt_stage_intersect_grid", primary_form == 0, n, origin, dir, t, normal, material, point,
                         [&](const ptd::Queues& qs, const int32_t* cnt, ptd::PathBuf pb, ptd::HitBuf hb) {
                           g.k->intersect_grid(g.stream, g.grid, tables(g), qs, cnt, pb, hb, primary_form != 0);
                         });
}

// The grid that pt_stage_intersect_grid walks, from the host copy of the uploaded cell table
int pt_stage_grid_info(PtGridInfo* info, int32_t* max_cell_records) {
  if (need(default_context(), "pt_stage_grid_info")) return -1;
  Ctx& g = *default_context();
  if (!info || !max_cell_records) return pt_fail("pt_stage_grid_info: null argument");
  const Ctx::DeviceGrid* gr = walked_grid(g);
  if (!gr) return pt_fail("pt_stage_grid_info: this context walks no grid (PtStats.grid_cells is 0; PtOptions.debug_flags 256 forces one)");
  if (grid_start_host(g, g.grids[g.grid_pick])) return -1;  // (a device build of the tables leaves the host copy to whoever asks)
  std::memset(info, 0, sizeof(*info));
  for (int a = 0; a < 3; ++a) info->res[a] = gr->shape.res[a], info->origin[a] = gr->shape.gmin[a], info->cell_size[a] = gr->shape.cs[a];
  info->pad = gr->shape.pad;
  const size_t cells = gr->start.size() - 1 - 2 * gr->guard;
  info->num_cells = (int32_t)cells;
  info->num_records = (int32_t)gr->start[gr->guard + cells];
  info->num_leaves = (g.scene.num_nodes + 1) / 2;
  uint32_t longest = 0;
  for (size_t c = 0; c < cells; ++c) longest = std::max(longest, gr->start[gr->guard + c + 1] - gr->start[gr->guard + c]);
  *max_cell_records = (int32_t)longest;
  return 0;
}

int pt_stage_read_tables(int which, void* out, uint64_t cap, uint64_t* bytes) {
  if (need(default_context(), "pt_stage_read_tables")) return -1;
  Ctx& g = *default_context();
  if (which < 0 || which > 8 || !bytes || (cap && !out)) return pt_fail("pt_stage_read_tables: bad argument");
  if (pt_ctx_sync(&g)) return -1;
  const ptk::SceneTables& s = g.scene;
  const Ctx::DeviceGrid* gr = g.grids.empty() ? nullptr : &g.grids[g.grid_pick];
  const bool copies = g.k->boxes_center_half != 0;
  const void* src = nullptr;
  size_t n = 0;
  switch (which) {
    case 0: src = s.nodes, n = (size_t)s.num_nodes * sizeof(ptd::Node); break;
    case 1: if (copies) src = s.nodes_b, n = (size_t)s.num_nodes * sizeof(ptd::Node); break;
    case 2: src = s.top, n = (size_t)s.num_top * sizeof(ptd::TopEntry); break;
    case 3: if (copies) src = s.top_b, n = (size_t)s.num_top * sizeof(ptd::TopEntry); break;
    case 4: if (gr) src = gr->d_start, n = gr->start.size() * sizeof(uint32_t); break;
    case 5: if (gr) src = gr->d_items, n = gr->items * sizeof(ptd::Node); break;
    case 6: if (gr && gr->d_items_b != gr->d_items) src = gr->d_items_b, n = gr->items * sizeof(ptd::Node); break;
    case 8: src = s.geoms, n = (size_t)s.num_geoms * sizeof(ptd::Geom); break;
    default: break;
  }
  if (which == 7) {
    *bytes = sizeof(float);
    if (cap) std::memcpy(out, &s.cull_margin, std::min<size_t>((size_t)cap, sizeof(float)));
    return 0;
  }
  *bytes = n;
  const size_t take = std::min<size_t>(n, (size_t)cap);
  if (take) HIP_OK(hipMemcpy(out, src, take, hipMemcpyDeviceToHost));
  return 0;
}

int pt_selfcheck_camera_math(int kind, uint64_t count, uint32_t seed, uint64_t* mismatches) {
  if (kind < 0 || kind >= ptct::kMathKinds || count > ((uint64_t)1 << 24) || !mismatches) return pt_fail("pt_selfcheck_camera_math: bad argument");
  return pt_camera_math_check(kind, count, seed, mismatches);
}

// The grid launches of move_tables_device (pt_api.cpp) on the caller's nodes, with that function's scalars and decisions for a forced grid
// (pt_tables.h device_grid_*); pt_camera_grid_host is the host side of the comparison.
int pt_stage_camera_grid(const PtTableNode* nodes, int num_nodes, const int32_t* geom_types, int num_geoms, const float root_min[3],
                         const float root_max[3], double coord_mag, const int32_t res[3], int center_half, PtCameraGridResult* out,
                         uint32_t* start, uint64_t start_cap, PtGridRecord* items, PtGridRecord* items_b, uint64_t items_cap) {
  const char* who = "pt_stage_camera_grid";
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  if (const char* why = pt::camera_grid_refusal(nodes, num_nodes, geom_types, num_geoms, root_min, root_max, coord_mag, res, out)) return pt_fail("%s: %s", who, why);
  const bool query = !start && !items;
  if (!query && (!start || !items || (center_half && !items_b))) return pt_fail("%s: null argument", who);
  ptct::BuildArgs a{};
  a.num_nodes = num_nodes, a.center_half = center_half ? 1 : 0;
  pt::GridShape shape{};
  int64_t ncell = 0;
  size_t guard = 0;
  const int want[3] = {res[0], res[1], res[2]};
  pt::GridVerdict v = pt::device_grid_scalars(root_min, root_max, coord_mag, want, num_geoms, a.frame, shape, &ncell, &guard);
  if (v != pt::kGridBuild) return pt::camera_grid_result(shape, guard, ncell, 0, 0, v, out), 0;  // nothing is launched
  a.ncell = (uint32_t)ncell, a.guard = (uint32_t)guard;
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  ptd::Node* d_nodes = nullptr;
  ptct::DeviceGeom* d_geoms = nullptr;
  std::vector<ptct::DeviceGeom> geoms((size_t)num_geoms, ptct::DeviceGeom{});
  for (int i = 0; i < num_geoms; ++i) geoms[(size_t)i].type = geom_types[i];
  if (device_copy(sc, who, reinterpret_cast<const ptd::Node*>(nodes), (size_t)num_nodes, &d_nodes) || device_copy(sc, who, geoms.data(), geoms.size(), &d_geoms)) return -1;
  ptct::BuildRecord* d_rec = sc.get<ptct::BuildRecord>(1);
  uint32_t* d_count = sc.get<uint32_t>((size_t)ncell);
  uint32_t* d_sums = sc.get<uint32_t>(pt_camera_tables_scan_blocks((size_t)ncell));
  if (!d_rec || !d_count || !d_sums) return pt_fail("%s: out of device memory", who);
  HIP_OK(hipMemsetAsync(d_rec, 0, sizeof(ptct::BuildRecord), g.stream));  // (pt_camera_tables_nodes_launch zeroes it for a renderer)
  if (pt_camera_tables_count_launch(g.stream, a, d_nodes, d_count, d_rec)) return -1;
  ptct::BuildRecord rec{};
  HIP_OK(hipMemcpyAsync(&rec, d_rec, sizeof(rec), hipMemcpyDeviceToHost, g.stream));
  HIP_OK(hipStreamSynchronize(g.stream));
  int64_t leaves = 0;
  for (int i = 0; i < num_nodes; ++i) leaves += nodes[i].geom >= 0 ? 1 : 0;
  v = pt::device_grid_counted(true, leaves, rec.refs, rec.longest, (size_t)ptct::kMaxRefs);
  pt::camera_grid_result(shape, guard, ncell, rec.refs, rec.longest, v, out);
  if (v != pt::kGridBuild || query) return 0;
  const size_t words = (size_t)ncell + 1 + 2 * guard, refs = (size_t)rec.refs;
  if (words > start_cap || refs > items_cap)
    return pt_fail("%s: the grid needs %zu words and %zu records, the arrays hold %llu and %llu", who, words, refs, (unsigned long long)start_cap,
                   (unsigned long long)items_cap);
  uint32_t* d_scratch = sc.get<uint32_t>(refs);
  uint32_t* d_start = sc.get<uint32_t>(words);
  ptd::Node* d_items = sc.get<ptd::Node>(refs);
  ptd::Node* d_items_b = center_half ? sc.get<ptd::Node>(refs) : nullptr;
  if (!d_scratch || !d_start || !d_items || (center_half && !d_items_b)) return pt_fail("%s: out of device memory", who);
  if (pt_camera_tables_grid_launch(g.stream, a, d_nodes, d_geoms, d_count, d_sums, d_scratch, (uint32_t)refs, d_start, d_items, d_items_b)) return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  HIP_OK(hipMemcpy(start, d_start, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(items, d_items, refs * sizeof(ptd::Node), hipMemcpyDeviceToHost));
  if (center_half) HIP_OK(hipMemcpy(items_b, d_items_b, refs * sizeof(ptd::Node), hipMemcpyDeviceToHost));
  return 0;
}

int pt_stage_shade(int n, int depth, const int32_t* iter, const int32_t* pixel, const float* t, const float* normal,
                   const int32_t* material, const float* point, float* origin, float* dir, float* color,
                   int32_t* alive) {
  if (need(default_context(), "pt_stage_shade")) return -1;
  Ctx& g = *default_context();
  if (n <= 0) return 0;
  if (depth < 0 || depth >= g.depth) return pt_fail("pt_stage_shade: depth %d outside [0,%d)", depth, g.depth);
  for (int i = 0; i < n; ++i)
    if (t[i] >= 0.0f && (material[i] < 0 || material[i] >= g.scene.num_mats))
      return pt_fail("pt_stage_shade: material id %d out of range at %d", material[i], i);
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const size_t cap = n;
  StagePaths sp;
  const bool have_paths = sp.alloc(sc, cap);
  ptd::HitBuf hb{};
  int32_t *d_iter = nullptr, *d_pix = nullptr, *d_alive = sc.get<int32_t>(cap);
  if (!have_paths || !scratch_hits(sc, cap, &hb) || !d_alive) return pt_fail("pt_stage_shade: out of device memory");
  const size_t b1 = (size_t)n * 4, b3 = 3 * b1;
  sp.pack(n, origin, dir, color);
  if (sp.upload()) return pt_fail("pt_stage_shade: upload failed");
  HIP_OK(hipMemcpy(hb.t, t, b1, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(hb.n, normal, b3, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(hb.mat, material, b1, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(hb.p, point, b3, hipMemcpyHostToDevice));
  if (device_copy(sc, "pt_stage_shade", iter, cap, &d_iter) || device_copy(sc, "pt_stage_shade", pixel, cap, &d_pix)) return -1;
  g.k->shade_stage(g.stream, tables(g), g.depth, depth, n, d_iter, d_pix, hb, sp.pb, d_alive);
  HIP_OK(hipStreamSynchronize(g.stream));
  if (sp.download()) return pt_fail("pt_stage_shade: download failed");
  sp.unpack(n, origin, dir, color);
  HIP_OK(hipMemcpy(alive, d_alive, b1, hipMemcpyDeviceToHost));
  return 0;
}

// k_save_u8 on a caller-supplied SUM image of whole rows (tests: pins the device conversion to the reference writer's bytes)
int pt_stage_save_u8(int w, int h, float samples, const float* rgb_sum, uint8_t* rgb8) {
  if (need(default_context(), "pt_stage_save_u8")) return -1;
  Ctx& g = *default_context();
  if (w <= 0 || h <= 0 || h >= 32768 || !rgb_sum || !rgb8 || !(samples > 0.0f)) return pt_fail("pt_stage_save_u8: bad argument");
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const size_t n = (size_t)w * h;
  float* d_img = nullptr;
  uint8_t* d_u8 = sc.get<uint8_t>(3 * n);
  if (!d_u8) return pt_fail("pt_stage_save_u8: out of device memory");
  if (device_copy(sc, "pt_stage_save_u8", rgb_sum, 3 * n, &d_img)) return -1;
  g.k->save_u8(g.stream, (int)n, w, samples, d_img, d_u8);
  HIP_OK(hipStreamSynchronize(g.stream));
  HIP_OK(hipMemcpy(rgb8, d_u8, 3 * n, hipMemcpyDeviceToHost));
  return 0;
}

// The filter kernels on caller-supplied host arrays (tests: frames a renderer would never produce): the resolved job `j` with the arrays
// filter_stage left on the device
static int filter_stage_job(Ctx& g, const char* who, int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, float* rgb_avg,
                            ptdn::Job& j) {
  return filter_stage(g, who, (size_t)w * rows, rgb_sum, planes, noise_planes, rgb_avg, [&](const float* img, const float* pl, const float* nz, void* ws, const float** out) {
    return j.f = {w, rows, img, pl, nz}, pt_denoise_launch(g.stream, j, ws, out);
  });
}
int pt_stage_denoise(int w, int rows, const float* rgb_sum, const float* planes, float samples, const PtDenoiseOptions* opt, float* rgb_avg) {
  if (need(default_context(), "pt_stage_denoise")) return -1;
  if (w <= 0 || rows <= 0 || rows >= 32768 || (int64_t)w * rows > (1ll << 30) || !rgb_sum || !planes || !rgb_avg) return pt_fail("pt_stage_denoise: bad argument");
  ptdn::Job j{};
  if (pt_denoise_resolve("pt_stage_denoise", ptdn::Form::Plain, samples, 0, 0, opt, &j)) return -1;
  return filter_stage_job(*default_context(), "pt_stage_denoise", w, rows, rgb_sum, planes, nullptr, rgb_avg, j);
}

// The guided filter's kernels on caller-supplied host arrays
int pt_stage_denoise_guided(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups, int64_t iters,
                            const PtDenoiseOptions* opt, float* rgb_avg) {
  if (need(default_context(), "pt_stage_denoise_guided")) return -1;
  if (w <= 0 || rows <= 0 || rows >= 32768 || (int64_t)w * rows > (1ll << 30) || !rgb_sum || !planes || !noise_planes || !rgb_avg)
    return pt_fail("pt_stage_denoise_guided: bad argument");
  ptdn::Job j{};
  if (pt_denoise_resolve("pt_stage_denoise_guided", ptdn::Form::Guided, 0.0f, groups, iters, opt, &j)) return -1;
  return filter_stage_job(*default_context(), "pt_stage_denoise_guided", w, rows, rgb_sum, planes, noise_planes, rgb_avg, j);
}

// The adaptive filter's kernels on caller-supplied host arrays (pt_denoise_adaptive_host's arguments); the counts travel beside the frame
int pt_stage_denoise_adaptive(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                              const PtDenoiseOptions* opt, float* rgb_avg) {
  if (need(default_context(), "pt_stage_denoise_adaptive")) return -1;
  Ctx& g = *default_context();
  if (rows >= 32768) return pt_fail("pt_stage_denoise_adaptive: a frame of %d x %d pixels is not supported", w, rows);
  if (!rgb_avg) return pt_fail("pt_stage_denoise_adaptive: null argument");
  ptdn::Job j{};
  if (pt_denoise_adaptive_check("pt_stage_denoise_adaptive", w, rows, rgb_sum, planes, noise_planes, counts, opt, &j)) return -1;
  Scratch counts_sc;  // (filter_stage synchronises before it returns)
  int32_t* d_counts = nullptr;
  HIP_OK(hipSetDevice(g.device));
  if (device_copy(counts_sc, "pt_stage_denoise_adaptive", counts, 2 * (size_t)w * rows, &d_counts)) return -1;
  j.div.cnt = reinterpret_cast<const ptad::Cnt*>(d_counts);
  return filter_stage_job(g, "pt_stage_denoise_adaptive", w, rows, rgb_sum, planes, noise_planes, rgb_avg, j);
}

// The reprojection's kernel on caller-supplied host arrays (pt_history_reproject_host's arguments)
int pt_stage_history_reproject(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                               const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, float* current_plane) {
  if (need(default_context(), "pt_stage_history_reproject")) return -1;
  Ctx& g = *default_context();
  pthi::Params P{};
  if (pt_history_reproject_check("pt_stage_history_reproject", w, rows, row0, kept_cam, kept_planes, feature_planes, reject_geom, num_geoms, opt, current_plane, &P))
    return -1;
  if (rows >= 32768) return pt_fail("pt_stage_history_reproject: a tile of %d x %d pixels is not supported", w, rows);
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const size_t n = (size_t)w * rows;
  float *d_kept = nullptr, *d_feat = nullptr;
  uint8_t* d_reject = nullptr;
  float* d_cur = sc.get<float>(4 * n);
  if (!d_cur) return pt_fail("pt_stage_history_reproject: out of device memory");
  if (device_copy(sc, "pt_stage_history_reproject", kept_planes, 4 * PT_HISTORY_KEPT_PLANES * n, &d_kept)) return -1;
  if (device_copy(sc, "pt_stage_history_reproject", feature_planes, 4 * PT_FEATURE_PLANES * n, &d_feat)) return -1;
  if (!P.keep_view_dependent && num_geoms > 0 && device_copy(sc, "pt_stage_history_reproject", reject_geom, (size_t)num_geoms, &d_reject)) return -1;
  HIP_OK(hipMemset(d_cur, 0xff, 4 * n * sizeof(float)));  // a pixel nobody wrote shows as NaNs
  if (pt_history_reproject_launch(g.stream, pthi::make_view(*kept_cam, rows, row0), d_kept, d_feat, d_reject, num_geoms, P, d_cur)) return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  HIP_OK(hipMemcpy(current_plane, d_cur, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// ... with the variance or the moments side (pt_history_reproject_variance_host's arguments): C and VC of one launch
static int stage_history_reproject_with(const char* who, bool moments, int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                        const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, float* current_plane,
                                        float* current_var) {
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  pthi::Params P{};
  if (pt_history_reproject_check(who, w, rows, row0, kept_cam, kept_planes, feature_planes, reject_geom, num_geoms, opt, current_plane, &P)) return -1;
  if (!kept_var || !current_var) return pt_fail("%s: null argument", who);
  if (rows >= 32768) return pt_fail("%s: a tile of %d x %d pixels is not supported", who, w, rows);
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const size_t n = (size_t)w * rows;
  float *d_kept = nullptr, *d_feat = nullptr, *d_kvar = nullptr;
  uint8_t* d_reject = nullptr;
  float* d_cur = sc.get<float>(8 * n);  // C, then VC
  if (!d_cur) return pt_fail("%s: out of device memory", who);
  if (device_copy(sc, who, kept_planes, 4 * PT_HISTORY_KEPT_PLANES * n, &d_kept) || device_copy(sc, who, feature_planes, 4 * PT_FEATURE_PLANES * n, &d_feat) ||
      device_copy(sc, who, kept_var, 4 * n, &d_kvar))
    return -1;
  if (!P.keep_view_dependent && num_geoms > 0 && device_copy(sc, who, reject_geom, (size_t)num_geoms, &d_reject)) return -1;
  HIP_OK(hipMemset(d_cur, 0xff, 8 * n * sizeof(float)));  // a pixel nobody wrote shows as NaNs
  if ((moments ? pt_history_reproject_moments_launch : pt_history_reproject_variance_launch)(g.stream, pthi::make_view(*kept_cam, rows, row0), d_kept, d_feat,
                                                                                            d_reject, num_geoms, P, d_cur, d_kvar, d_cur + 4 * n))
    return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  HIP_OK(hipMemcpy(current_plane, d_cur, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(current_var, d_cur + 4 * n, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int pt_stage_history_reproject_variance(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                        const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, float* current_plane,
                                        float* current_var) {
  return stage_history_reproject_with("pt_stage_history_reproject_variance", false, w, rows, row0, kept_cam, kept_planes, feature_planes, reject_geom, num_geoms, opt, kept_var,
                                      current_plane, current_var);
}
int pt_stage_history_reproject_moments(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                       const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, float* current_plane,
                                       float* current_var) {
  return stage_history_reproject_with("pt_stage_history_reproject_moments", true, w, rows, row0, kept_cam, kept_planes, feature_planes, reject_geom, num_geoms, opt, kept_var,
                                      current_plane, current_var);
}

// ... with the objects' motion (pt_history_reproject_motion_host's arguments): k_history_reproject_motion of the kind `flags` names
int pt_stage_history_reproject_motion(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                      const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, const float* table,
                                      const uint8_t* kind, uint32_t flags, float* current_plane, float* current_var) {
  const char* who = "pt_stage_history_reproject_motion";
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  pthi::Params P{};
  if (pt_history_reproject_check(who, w, rows, row0, kept_cam, kept_planes, feature_planes, reject_geom, num_geoms, opt, current_plane, &P)) return -1;
  if (pt_history_motion_check(who, flags, num_geoms, table, kind, kept_var, current_var)) return -1;
  if (rows >= 32768) return pt_fail("%s: a tile of %d x %d pixels is not supported", who, w, rows);
  const uint32_t with = flags & (PT_HISTORY_VARIANCE | PT_HISTORY_MOMENTS);
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const size_t n = (size_t)w * rows;
  float *d_kept = nullptr, *d_feat = nullptr, *d_kvar = nullptr, *d_table = nullptr;
  uint8_t *d_reject = nullptr, *d_kind = nullptr;
  float* d_cur = sc.get<float>(8 * n);  // C, then VC
  if (!d_cur) return pt_fail("%s: out of device memory", who);
  if (device_copy(sc, who, kept_planes, 4 * PT_HISTORY_KEPT_PLANES * n, &d_kept) || device_copy(sc, who, feature_planes, 4 * PT_FEATURE_PLANES * n, &d_feat) ||
      device_copy(sc, who, table, (size_t)pthi::kMotionRow * num_geoms, &d_table) || device_copy(sc, who, kind, (size_t)num_geoms, &d_kind))
    return -1;
  if (with && device_copy(sc, who, kept_var, 4 * n, &d_kvar)) return -1;
  if (!P.keep_view_dependent && device_copy(sc, who, reject_geom, (size_t)num_geoms, &d_reject)) return -1;
  HIP_OK(hipMemset(d_cur, 0xff, 8 * n * sizeof(float)));  // a pixel nobody wrote shows as NaNs
  if (pt_history_reproject_motion_launch(g.stream, with, pthi::make_view(*kept_cam, rows, row0), d_kept, d_feat, d_reject, num_geoms, P, d_cur, d_kvar,
                                         with ? d_cur + 4 * n : nullptr, d_table, d_kind))
    return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  HIP_OK(hipMemcpy(current_plane, d_cur, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
  if (with) HIP_OK(hipMemcpy(current_var, d_cur + 4 * n, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// ... with the materials' edits (pt_history_reproject_materials_host's arguments): k_history_reproject_materials of the kind `flags` names
int pt_stage_history_reproject_materials(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                         const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, const float* table,
                                         const uint8_t* kind, const float* recolor, const uint8_t* rkind, uint32_t flags, float* current_plane, float* current_var) {
  const char* who = "pt_stage_history_reproject_materials";
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  pthi::Params P{};
  if (pt_history_reproject_check(who, w, rows, row0, kept_cam, kept_planes, feature_planes, reject_geom, num_geoms, opt, current_plane, &P)) return -1;
  if (pt_history_materials_check(who, flags, num_geoms, table, kind, recolor, rkind, kept_var, current_var)) return -1;
  if (rows >= 32768) return pt_fail("%s: a tile of %d x %d pixels is not supported", who, w, rows);
  const uint32_t with = flags & (PT_HISTORY_VARIANCE | PT_HISTORY_MOMENTS);
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const size_t n = (size_t)w * rows;
  float *d_kept = nullptr, *d_feat = nullptr, *d_kvar = nullptr, *d_table = nullptr, *d_recolor = nullptr;
  uint8_t *d_reject = nullptr, *d_kind = nullptr, *d_rkind = nullptr;
  float* d_cur = sc.get<float>(8 * n);  // C, then VC
  if (!d_cur) return pt_fail("%s: out of device memory", who);
  if (device_copy(sc, who, kept_planes, 4 * PT_HISTORY_KEPT_PLANES * n, &d_kept) || device_copy(sc, who, feature_planes, 4 * PT_FEATURE_PLANES * n, &d_feat) ||
      device_copy(sc, who, recolor, (size_t)pthi::kRecolorRow * num_geoms, &d_recolor) || device_copy(sc, who, rkind, (size_t)num_geoms, &d_rkind))
    return -1;
  if (table && (device_copy(sc, who, table, (size_t)pthi::kMotionRow * num_geoms, &d_table) || device_copy(sc, who, kind, (size_t)num_geoms, &d_kind))) return -1;
  if (with && device_copy(sc, who, kept_var, 4 * n, &d_kvar)) return -1;
  if (!P.keep_view_dependent && device_copy(sc, who, reject_geom, (size_t)num_geoms, &d_reject)) return -1;
  HIP_OK(hipMemset(d_cur, 0xff, 8 * n * sizeof(float)));  // a pixel nobody wrote shows as NaNs
  if (pt_history_reproject_materials_launch(g.stream, with, pthi::make_view(*kept_cam, rows, row0), d_kept, d_feat, d_reject, num_geoms, P, d_cur, d_kvar,
                                            with ? d_cur + 4 * n : nullptr, d_table, d_kind, d_recolor, d_rkind))
    return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  HIP_OK(hipMemcpy(current_plane, d_cur, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
  if (with) HIP_OK(hipMemcpy(current_var, d_cur + 4 * n, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// The history filter's kernels on caller-supplied host arrays (pt_history_denoise_host's arguments); C and VC travel beside the frame
int pt_stage_history_denoise(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups, int64_t iters, float samples,
                             const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, float* rgb_avg) {
  const char* who = "pt_stage_history_denoise";
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  if (rows >= 32768) return pt_fail("%s: a frame of %d x %d pixels is not supported", who, w, rows);
  ptdn::Job j{};
  if (pt_history_denoise_check(who, w, rows, rgb_sum, planes, noise_planes, groups, iters, samples, current_plane, current_var, opt, rgb_avg, &j)) return -1;
  Scratch hist_sc;  // (filter_stage synchronises before it returns)
  float *d_cur = nullptr, *d_var = nullptr;
  HIP_OK(hipSetDevice(g.device));
  const size_t n = (size_t)w * rows;
  if (current_plane && (device_copy(hist_sc, who, current_plane, 4 * n, &d_cur) || device_copy(hist_sc, who, current_var, 4 * n, &d_var))) return -1;
  j.div.C = reinterpret_cast<const ptdn::V4*>(d_cur), j.div.VC = reinterpret_cast<const ptdn::V4*>(d_var);
  return filter_stage_job(g, who, w, rows, rgb_sum, planes, noise_planes, rgb_avg, j);
}

// ... and the moments form's (pt_history_denoise_moments_host's arguments but its optional outputs)
int pt_stage_history_denoise_moments(int w, int rows, const float* rgb_sum, const float* planes, float samples, const float* current_plane,
                                     const float* current_var, const PtDenoiseOptions* opt, float* rgb_avg) {
  const char* who = "pt_stage_history_denoise_moments";
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  if (rows >= 32768) return pt_fail("%s: a frame of %d x %d pixels is not supported", who, w, rows);
  ptdn::Job j{};
  if (pt_history_denoise_moments_check(who, w, rows, rgb_sum, planes, samples, current_plane, current_var, opt, rgb_avg != nullptr, &j)) return -1;
  Scratch hist_sc;  // (filter_stage synchronises before it returns)
  float *d_cur = nullptr, *d_var = nullptr;
  HIP_OK(hipSetDevice(g.device));
  const size_t n = (size_t)w * rows;
  if (current_plane && (device_copy(hist_sc, who, current_plane, 4 * n, &d_cur) || device_copy(hist_sc, who, current_var, 4 * n, &d_var))) return -1;
  j.div.C = reinterpret_cast<const ptdn::V4*>(d_cur), j.div.VC = reinterpret_cast<const ptdn::V4*>(d_var);
  return filter_stage_job(g, who, w, rows, rgb_sum, planes, nullptr, rgb_avg, j);
}

// ... and the feedback form's (pt_history_denoise_feedback_host's arguments but var_raw and mark): the prepare with FC (counted when
// `extra` is given), the moments form's kernels, the tap after level fb->level - 1; rgb_avg and tap, either may be null but not both
int pt_stage_history_denoise_feedback(int w, int rows, const float* rgb_sum, const float* planes, float samples, const float* extra, const float* current_plane,
                                      const float* current_var, const float* current_fb, const PtDenoiseOptions* opt, const PtHistoryFeedbackOptions* fb,
                                      float* rgb_avg, float* tap) {
  const char* who = "pt_stage_history_denoise_feedback";
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  if (rows >= 32768) return pt_fail("%s: a frame of %d x %d pixels is not supported", who, w, rows);
  ptdn::Job j{};
  if (pt_history_denoise_feedback_check(who, w, rows, rgb_sum, planes, samples, current_plane, current_var, current_fb, opt, fb, rgb_avg || tap, &j)) return -1;
  const size_t n = (size_t)w * rows;
  if (extra && pt_history_check_extra(who, (int)n, extra)) return -1;
  Scratch hist_sc;  // (filter_stage synchronises before it returns)
  float *d_cur = nullptr, *d_var = nullptr, *d_fb = nullptr, *d_extra = nullptr;
  HIP_OK(hipSetDevice(g.device));
  float* d_tap = hist_sc.get<float>(4 * n);
  if (!d_tap) return pt_fail("%s: out of device memory", who);
  HIP_OK(hipMemset(d_tap, 0xff, 4 * n * sizeof(float)));  // a pixel nobody wrote shows as NaNs
  if (current_plane && (device_copy(hist_sc, who, current_plane, 4 * n, &d_cur) || device_copy(hist_sc, who, current_var, 4 * n, &d_var) ||
                        device_copy(hist_sc, who, current_fb, 4 * n, &d_fb)))
    return -1;
  if (extra && device_copy(hist_sc, who, extra, n, &d_extra)) return -1;
  j.div.C = reinterpret_cast<const ptdn::V4*>(d_cur), j.div.VC = reinterpret_cast<const ptdn::V4*>(d_var), j.div.FC = reinterpret_cast<const ptdn::V4*>(d_fb);
  j.div.E = d_extra;
  j.tap = d_tap;
  std::vector<float> avg(rgb_avg ? 0 : 3 * n);  // (filter_stage writes an image)
  if (filter_stage_job(g, who, w, rows, rgb_sum, planes, nullptr, rgb_avg ? rgb_avg : avg.data(), j)) return -1;
  if (tap) HIP_OK(hipMemcpy(tap, d_tap, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// The lookup with the filtered colour on caller-supplied host arrays (pt_history_reproject_feedback_host's arguments)
int pt_stage_history_reproject_feedback(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                        const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, const float* kept_fb,
                                        const float* table, const uint8_t* kind, float* current_plane, float* current_var, float* current_fb) {
  const char* who = "pt_stage_history_reproject_feedback";
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  pthi::Params P{};
  if (pt_history_reproject_check(who, w, rows, row0, kept_cam, kept_planes, feature_planes, reject_geom, num_geoms, opt, current_plane, &P)) return -1;
  if (pt_history_reproject_feedback_check(who, num_geoms, kept_var, kept_fb, table, kind, current_var, current_fb)) return -1;
  if (rows >= 32768) return pt_fail("%s: a tile of %d x %d pixels is not supported", who, w, rows);
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const size_t n = (size_t)w * rows;
  float *d_kept = nullptr, *d_feat = nullptr, *d_kvar = nullptr, *d_kfb = nullptr, *d_table = nullptr;
  uint8_t *d_reject = nullptr, *d_kind = nullptr;
  float* d_cur = sc.get<float>(12 * n);  // C, then VC, then FC
  if (!d_cur) return pt_fail("%s: out of device memory", who);
  if (device_copy(sc, who, kept_planes, 4 * PT_HISTORY_KEPT_PLANES * n, &d_kept) || device_copy(sc, who, feature_planes, 4 * PT_FEATURE_PLANES * n, &d_feat) ||
      device_copy(sc, who, kept_var, 4 * n, &d_kvar) || device_copy(sc, who, kept_fb, 4 * n, &d_kfb))
    return -1;
  if (table && (device_copy(sc, who, table, (size_t)pthi::kMotionRow * num_geoms, &d_table) || device_copy(sc, who, kind, (size_t)num_geoms, &d_kind))) return -1;
  if (!P.keep_view_dependent && num_geoms > 0 && device_copy(sc, who, reject_geom, (size_t)num_geoms, &d_reject)) return -1;
  HIP_OK(hipMemset(d_cur, 0xff, 12 * n * sizeof(float)));  // a pixel nobody wrote shows as NaNs
  if (pt_history_reproject_feedback_launch(g.stream, pthi::make_view(*kept_cam, rows, row0), d_kept, d_feat, d_reject, num_geoms, P, d_cur, d_kvar, d_cur + 4 * n,
                                           d_kfb, d_cur + 8 * n, d_table, d_kind))
    return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  HIP_OK(hipMemcpy(current_plane, d_cur, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(current_var, d_cur + 4 * n, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(current_fb, d_cur + 8 * n, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// The selection's kernels on caller-supplied host arrays (pt_adaptive_select_host's arguments)
int pt_stage_adaptive_select(int w, int rows, const float* noise_planes, const int32_t* counts, int m, int32_t* list) {
  if (need(default_context(), "pt_stage_adaptive_select")) return -1;
  Ctx& g = *default_context();
  if (pt_adaptive_check_select("pt_stage_adaptive_select", w, rows, noise_planes, counts, m, list)) return -1;
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const size_t n = (size_t)w * rows;
  float* d_plane0 = nullptr;
  int32_t* d_counts = nullptr;
  char* d_ws = sc.get<char>(pt_adaptive_select_bytes(n));
  int32_t* d_list = sc.get<int32_t>((size_t)m);
  if (!d_ws || !d_list) return pt_fail("pt_stage_adaptive_select: out of device memory");
  if (device_copy(sc, "pt_stage_adaptive_select", noise_planes, 4 * n, &d_plane0)) return -1;  // the selection reads plane 0 only
  if (device_copy(sc, "pt_stage_adaptive_select", counts, 2 * n, &d_counts)) return -1;
  HIP_OK(hipMemset(d_list, 0xff, (size_t)m * sizeof(int32_t)));  // an entry nobody wrote shows as -1
  if (pt_adaptive_select_launch(g.stream, w, rows, d_plane0, d_counts, m, d_ws, d_list)) return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  HIP_OK(hipMemcpy(list, d_list, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
  return 0;
}

// The threshold selection's kernels on caller-supplied host arrays (pt_adaptive_select_threshold_host's arguments)
int pt_stage_adaptive_select_threshold(int w, int rows, const float* noise_planes, const int32_t* counts, float threshold, int cap, int32_t* list,
                                       int* above, int* m) {
  if (need(default_context(), "pt_stage_adaptive_select_threshold")) return -1;
  Ctx& g = *default_context();
  if (pt_adaptive_check_select("pt_stage_adaptive_select_threshold", w, rows, noise_planes, counts, cap, list)) return -1;
  if (pt_adaptive_check_threshold("pt_stage_adaptive_select_threshold", threshold)) return -1;
  if (!above || !m) return pt_fail("pt_stage_adaptive_select_threshold: bad argument");
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const size_t n = (size_t)w * rows;
  float* d_plane0 = nullptr;
  int32_t* d_counts = nullptr;
  char* d_ws = sc.get<char>(pt_adaptive_select_bytes(n));
  int32_t* d_list = sc.get<int32_t>((size_t)cap);
  if (!d_ws || !d_list) return pt_fail("pt_stage_adaptive_select_threshold: out of device memory");
  if (device_copy(sc, "pt_stage_adaptive_select_threshold", noise_planes, 4 * n, &d_plane0)) return -1;  // the selection reads plane 0 only
  if (device_copy(sc, "pt_stage_adaptive_select_threshold", counts, 2 * n, &d_counts)) return -1;
  HIP_OK(hipMemset(d_list, 0xff, (size_t)cap * sizeof(int32_t)));  // an entry nobody wrote shows as -1
  if (pt_adaptive_select_threshold_launch(g.stream, w, rows, d_plane0, d_counts, threshold, cap, d_ws, d_list)) return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  uint32_t result[2] = {0u, 0u};
  HIP_OK(hipMemcpy(result, pt_adaptive_select_result(d_ws, n), sizeof(result), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(list, d_list, (size_t)cap * sizeof(int32_t), hipMemcpyDeviceToHost));  // all cap entries: those behind m must still be -1
  *above = (int)result[0], *m = (int)result[1];
  return 0;
}

// The history round's key and selection on caller-supplied host arrays (pt_history_select_host's arguments): the key kernel writes into
// the selection's workspace, the selection is the round's own launch.
int pt_stage_history_select(int w, int rows, const float* feature_planes, const float* current_plane, const uint8_t* emitter_geom, int num_geoms,
                            const PtHistoryRoundOptions* opt, int32_t* list, int* fresh, int* m) {
  const char* who = "pt_stage_history_select";
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  pthi::RoundParams P{};
  int cap = 0;
  if (pt_history_select_check(who, w, rows, feature_planes, emitter_geom, num_geoms, opt, list, fresh, m, &P, &cap)) return -1;
  if (rows >= 32768) return pt_fail("%s: a tile of %d x %d pixels is not supported", who, w, rows);
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const size_t n = (size_t)w * rows;
  float *d_feat = nullptr, *d_cur = nullptr;
  uint8_t* d_emitter = nullptr;
  char* d_ws = sc.get<char>(pt_adaptive_select_bytes(n));
  int32_t* d_list = sc.get<int32_t>((size_t)cap);
  if (!d_ws || !d_list) return pt_fail("%s: out of device memory", who);
  if (device_copy(sc, who, feature_planes, 4 * PT_FEATURE_PLANES * n, &d_feat)) return -1;
  if (current_plane && device_copy(sc, who, current_plane, 4 * n, &d_cur)) return -1;
  if (num_geoms > 0 && device_copy(sc, who, emitter_geom, (size_t)num_geoms, &d_emitter)) return -1;
  HIP_OK(hipMemset(d_list, 0xff, (size_t)cap * sizeof(int32_t)));  // an entry nobody wrote shows as -1
  if (pt_history_key_launch(g.stream, (int)n, d_feat, d_cur, d_emitter, num_geoms, P.min_history, pt_adaptive_select_keys(d_ws, n))) return -1;
  if (pt_adaptive_select_threshold_keys_launch(g.stream, w, rows, 0.0f, cap, d_ws, d_list)) return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  uint32_t result[2] = {0u, 0u};
  HIP_OK(hipMemcpy(result, pt_adaptive_select_result(d_ws, n), sizeof(result), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(list, d_list, (size_t)cap * sizeof(int32_t), hipMemcpyDeviceToHost));  // all cap entries: those behind m must still be -1
  *fresh = (int)result[0], *m = (int)result[1];
  return 0;
}

// ... and its merge (pt_history_merge_host's arguments): rgb_sum and extra go up, through the kernel and come back.
int pt_stage_history_merge(int pixels, float* rgb_sum, float* extra, const int32_t* list, int m, const float* group_sum, int group_iters) {
  const char* who = "pt_stage_history_merge";
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  if (pt_history_merge_check(who, pixels, rgb_sum, extra, list, m, group_sum, group_iters)) return -1;
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  float *d_img = nullptr, *d_extra = nullptr, *d_sw = nullptr;
  int32_t* d_list = nullptr;
  if (device_copy(sc, who, rgb_sum, 3 * (size_t)pixels, &d_img) || device_copy(sc, who, extra, (size_t)pixels, &d_extra) ||
      device_copy(sc, who, group_sum, 3 * (size_t)m, &d_sw) || device_copy(sc, who, list, (size_t)m, &d_list))
    return -1;
  if (pt_history_merge_launch(g.stream, pixels, d_img, d_extra, d_list, m, d_sw, group_iters)) return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  HIP_OK(hipMemcpy(rgb_sum, d_img, 3 * (size_t)pixels * sizeof(float), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(extra, d_extra, (size_t)pixels * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// The estimate of the blend's noise on caller-supplied host arrays (pt_history_noise_host's arguments): k_history_noise and the reduction
int pt_stage_history_noise(int pixels, const float* noise_planes, int groups, int64_t iters, float samples, const float* current_plane, const float* current_var,
                           float* w_out, double* sse) {
  const char* who = "pt_stage_history_noise";
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  if (pt_history_noise_check(who, pixels, noise_planes, groups, iters, samples, current_plane, current_var)) return -1;
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const size_t n = (size_t)pixels;
  float *d_noise = nullptr, *d_cur = nullptr, *d_var = nullptr;
  char* d_out = sc.get<char>(pt_history_noise_bytes(n));
  if (!d_out) return pt_fail("%s: out of device memory", who);
  if (device_copy(sc, who, noise_planes, 4 * PT_NOISE_PLANES * n, &d_noise)) return -1;
  if (current_plane && (device_copy(sc, who, current_plane, 4 * n, &d_cur) || device_copy(sc, who, current_var, 4 * n, &d_var))) return -1;
  HIP_OK(hipMemsetAsync(d_out, 0xff, pt_history_noise_bytes(n), g.stream));  // a word nobody wrote shows as a NaN (on the kernels' stream: ordered before them)
  const ptnz::Fold f = ptnz::fold_scalars(1, groups, iters);
  if (pt_history_noise_launch(g.stream, pixels, d_noise, f.Tf, f.Df, samples, d_cur, d_var, d_out)) return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  if (w_out) HIP_OK(hipMemcpy(w_out, pt_history_noise_plane(d_out, n), n * sizeof(float), hipMemcpyDeviceToHost));
  if (sse) HIP_OK(hipMemcpy(sse, pt_history_noise_result(d_out, n), sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// ---- threshold rounds over the blend on caller-supplied host arrays (pt_history_threshold.hip; the *_host twins' arguments) ----------
namespace {
// counts, C and VC on the device; C and VC stay nullptr when absent
struct BlendInputs {
  int32_t* counts = nullptr;
  float *cur = nullptr, *var = nullptr;
};
int blend_inputs(Scratch& sc, const char* who, size_t n, const int32_t* counts, const float* current_plane, const float* current_var, BlendInputs* in) {
  if (device_copy(sc, who, counts, 2 * n, &in->counts)) return -1;
  if (current_plane && (device_copy(sc, who, current_plane, 4 * n, &in->cur) || device_copy(sc, who, current_var, 4 * n, &in->var))) return -1;
  return 0;
}
}  // namespace

// Pass A and the reduction: W, NE and the double.
int pt_stage_history_noise_adaptive(int pixels, const float* noise_planes, const int32_t* counts, const float* current_plane, const float* current_var,
                                    float* w_out, float* ne_out, double* sse) {
  const char* who = "pt_stage_history_noise_adaptive";
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  if (pixels <= 0 || pixels > (1 << 30) || !noise_planes) return pt_fail("%s: bad argument", who);
  if (pt_history_counts_check(who, pixels, counts, current_plane, current_var)) return -1;
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const size_t n = (size_t)pixels;
  float* d_noise = nullptr;
  BlendInputs in;
  char* d_out = sc.get<char>(pt_history_noise_bytes(n));
  float* d_ne = sc.get<float>(n);
  if (!d_out || !d_ne) return pt_fail("%s: out of device memory", who);
  if (device_copy(sc, who, noise_planes, 4 * PT_NOISE_PLANES * n, &d_noise) || blend_inputs(sc, who, n, counts, current_plane, current_var, &in)) return -1;
  HIP_OK(hipMemsetAsync(d_out, 0xff, pt_history_noise_bytes(n), g.stream));  // a word nobody wrote shows as a NaN
  HIP_OK(hipMemsetAsync(d_ne, 0xff, n * sizeof(float), g.stream));
  if (pt_history_noise_counts_launch(g.stream, pixels, d_noise, in.counts, 0, 0, in.cur, in.var, d_out, d_ne, true)) return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  if (w_out) HIP_OK(hipMemcpy(w_out, pt_history_noise_plane(d_out, n), n * sizeof(float), hipMemcpyDeviceToHost));
  if (ne_out) HIP_OK(hipMemcpy(ne_out, d_ne, n * sizeof(float), hipMemcpyDeviceToHost));
  if (sse) HIP_OK(hipMemcpy(sse, pt_history_noise_result(d_out, n), sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// Passes A and B into the selection's workspace, then the round's own selection launches.
int pt_stage_history_select_threshold_blend(int w, int rows, const float* noise_planes, const int32_t* counts, const float* current_plane, const float* current_var,
                                            float threshold, int cap, int32_t* list, int* above, int* m) {
  const char* who = "pt_stage_history_select_threshold_blend";
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  if (pt_adaptive_check_select(who, w, rows, noise_planes, counts, cap, list)) return -1;
  if (pt_adaptive_check_threshold(who, threshold)) return -1;
  if (!above || !m) return pt_fail("%s: bad argument", who);
  if (pt_history_counts_check(who, w * rows, counts, current_plane, current_var)) return -1;
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const size_t n = (size_t)w * rows;
  float* d_noise = nullptr;
  BlendInputs in;
  char* d_out = sc.get<char>(pt_history_noise_bytes(n));
  float* d_ne = sc.get<float>(n);
  char* d_ws = sc.get<char>(pt_adaptive_select_bytes(n));
  int32_t* d_list = sc.get<int32_t>((size_t)cap);
  if (!d_out || !d_ne || !d_ws || !d_list) return pt_fail("%s: out of device memory", who);
  if (device_copy(sc, who, noise_planes, 4 * PT_NOISE_PLANES * n, &d_noise) || blend_inputs(sc, who, n, counts, current_plane, current_var, &in)) return -1;
  HIP_OK(hipMemset(d_list, 0xff, (size_t)cap * sizeof(int32_t)));  // an entry nobody wrote shows as -1
  if (pt_history_noise_counts_launch(g.stream, (int)n, d_noise, in.counts, 0, 0, in.cur, in.var, d_out, d_ne, false)) return -1;
  if (pt_history_key_blend_launch(g.stream, w, rows, pt_history_noise_plane(d_out, n), d_ne, pt_adaptive_select_keys(d_ws, n))) return -1;
  if (pt_adaptive_select_threshold_keys_launch(g.stream, w, rows, threshold, cap, d_ws, d_list)) return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  uint32_t result[2] = {0u, 0u};
  HIP_OK(hipMemcpy(result, pt_adaptive_select_result(d_ws, n), sizeof(result), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(list, d_list, (size_t)cap * sizeof(int32_t), hipMemcpyDeviceToHost));  // all cap entries: those behind m must still be -1
  *above = (int)result[0], *m = (int)result[1];
  return 0;
}

// The capture and the blend: K, VK and (rgb_avg, may be NULL) the resolve.
int pt_stage_history_capture_adaptive(int pixels, const float* rgb_sum, const float* feature_planes, const float* noise_planes, const int32_t* counts,
                                      const float* current_plane, const float* current_var, float* kept_planes, float* kept_var, float* rgb_avg) {
  const char* who = "pt_stage_history_capture_adaptive";
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  if (pixels <= 0 || pixels > (1 << 30) || !rgb_sum || !feature_planes || !noise_planes || !kept_planes || !kept_var) return pt_fail("%s: bad argument", who);
  if (pt_history_counts_check(who, pixels, counts, current_plane, current_var)) return -1;
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const size_t n = (size_t)pixels;
  float *d_img = nullptr, *d_feat = nullptr, *d_noise = nullptr;
  BlendInputs in;
  float* d_kept = sc.get<float>(4 * PT_HISTORY_KEPT_PLANES * n);
  float* d_kvar = sc.get<float>(4 * n);
  float* d_avg = sc.get<float>(3 * n);
  if (!d_kept || !d_kvar || !d_avg) return pt_fail("%s: out of device memory", who);
  if (device_copy(sc, who, rgb_sum, 3 * n, &d_img) || device_copy(sc, who, feature_planes, 4 * PT_FEATURE_PLANES * n, &d_feat) ||
      device_copy(sc, who, noise_planes, 4 * PT_NOISE_PLANES * n, &d_noise) || blend_inputs(sc, who, n, counts, current_plane, current_var, &in))
    return -1;
  HIP_OK(hipMemsetAsync(d_kept, 0xff, 4 * PT_HISTORY_KEPT_PLANES * n * sizeof(float), g.stream));
  HIP_OK(hipMemsetAsync(d_kvar, 0xff, 4 * n * sizeof(float), g.stream));
  HIP_OK(hipMemsetAsync(d_avg, 0xff, 3 * n * sizeof(float), g.stream));
  if (pt_history_capture_counts_launch(g.stream, pixels, d_img, d_feat, d_noise, in.counts, 0, 0, in.cur, in.var, d_kept, d_kvar)) return -1;
  if (pt_history_blend_counts_launch(g.stream, pixels, d_img, in.counts, 0, 0, in.cur, d_avg)) return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  HIP_OK(hipMemcpy(kept_planes, d_kept, 4 * PT_HISTORY_KEPT_PLANES * n * sizeof(float), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(kept_var, d_kvar, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
  if (rgb_avg) HIP_OK(hipMemcpy(rgb_avg, d_avg, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// The filter over the blend with per-pixel counts (pt_history_denoise_adaptive_host's arguments)
int pt_stage_history_denoise_adaptive(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                                      const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, float* rgb_avg) {
  const char* who = "pt_stage_history_denoise_adaptive";
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  if (rows >= 32768) return pt_fail("%s: a frame of %d x %d pixels is not supported", who, w, rows);
  ptdn::Job j{};
  if (pt_history_denoise_adaptive_check(who, w, rows, rgb_sum, planes, noise_planes, counts, current_plane, current_var, opt, rgb_avg != nullptr, &j)) return -1;
  Scratch in_sc;  // (filter_stage synchronises before it returns)
  BlendInputs in;
  HIP_OK(hipSetDevice(g.device));
  if (blend_inputs(in_sc, who, (size_t)w * rows, counts, current_plane, current_var, &in)) return -1;
  j.div.cnt = reinterpret_cast<const ptad::Cnt*>(in.counts);
  j.div.C = reinterpret_cast<const ptdn::V4*>(in.cur), j.div.VC = reinterpret_cast<const ptdn::V4*>(in.var);
  return filter_stage_job(g, who, w, rows, rgb_sum, planes, noise_planes, rgb_avg, j);
}

// The partition's kernels on caller-supplied host arrays (pt_group_partition_host's arguments).  The list's length reaches the kernels
// as it does in a group's round: in the second of two words on the device.
int pt_stage_group_partition(int w, int h, int n, const int32_t* list, int m, int32_t* parts, int32_t* counts) {
  if (need(default_context(), "pt_stage_group_partition")) return -1;
  Ctx& g = *default_context();
  if (pt_group_partition_check("pt_stage_group_partition", w, h, n, list, m, parts, counts)) return -1;
  HIP_OK(hipSetDevice(g.device));
  Scratch sc;
  const int entries = std::max(m, 1);
  int32_t* d_list = sc.get<int32_t>((size_t)entries);
  int32_t* d_parts = sc.get<int32_t>((size_t)entries);
  uint32_t* d_words = sc.get<uint32_t>(2 + 2 + (size_t)n);  // {above, m} as the selection leaves them | the partition's result
  char* d_ws = sc.get<char>(pt_group_partition_bytes((size_t)entries, n));
  if (!d_list || !d_parts || !d_words || !d_ws) return pt_fail("pt_stage_group_partition: out of device memory");
  const uint32_t sel[2] = {(uint32_t)m, (uint32_t)m};
  HIP_OK(hipMemcpy(d_words, sel, sizeof(sel), hipMemcpyHostToDevice));
  if (m) HIP_OK(hipMemcpy(d_list, list, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_OK(hipMemset(d_parts, 0xff, (size_t)entries * sizeof(int32_t)));  // an entry nobody wrote shows as -1
  if (pt_group_partition_launch(g.stream, w, n, d_list, d_words, entries, d_ws, d_parts, d_words + 2)) return -1;
  HIP_OK(hipStreamSynchronize(g.stream));
  std::vector<uint32_t> result(2 + (size_t)n);
  HIP_OK(hipMemcpy(result.data(), d_words + 2, result.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (m) HIP_OK(hipMemcpy(parts, d_parts, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (result[0] != (uint32_t)m || result[1] != (uint32_t)m) return pt_fail("pt_stage_group_partition: the kernels read a list of %u, not %d", result[1], m);
  for (int i = 0; i < n; ++i) counts[i] = (int32_t)result[2 + (size_t)i];
  return 0;
}

// The worker context alone: iterations iter_first .. iter_first + iter_count - 1 of the m listed tile pixels (distinct, any order);
// rgb_sum_host receives the group sum, m * 3 floats in list order.  Leaves image, folds and state of the renderer alone.
static int stage_render_list(const char* who, const int32_t* list, int m, int capacity, int iter_first, int iter_count, float* rgb_sum_host) {
  if (need(default_context(), who)) return -1;
  Ctx& g = *default_context();
  if (!list || !rgb_sum_host || m < 1 || m > capacity || capacity > g.N || iter_first < 1 || iter_count < 0 || (int64_t)iter_first + iter_count - 1 > INT32_MAX)
    return pt_fail("%s: bad argument (a list of %d, a worker for %d out of %d pixels, iterations %d, +%d)", who, m, capacity, g.N, iter_first, iter_count);
  if (admit(g, who, kNotFailed)) return -1;
  if (g.stripe) return pt_fail("%s: a striped tile has no list form", who);
  {
    std::vector<uint8_t> seen((size_t)g.N, 0);
    for (int i = 0; i < m; ++i) {
      if (list[i] < 0 || list[i] >= g.N || seen[(size_t)list[i]]) return pt_fail("%s: list[%d] = %d is outside the tile or repeated", who, i, list[i]);
      seen[(size_t)list[i]] = 1;
    }
  }
  HIP_OK(hipSetDevice(g.device));
  if (ensure_worker(g, capacity)) return -1;
  set_worker_live(*g.worker, m);
  HIP_OK(hipStreamSynchronize(g.stream));  // (the list may still be read by an earlier round)
  HIP_OK(hipMemcpy(g.d_list, list, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice));
  if (render_list(g, iter_first, iter_count)) return -1;
  HIP_OK(hipMemcpyAsync(rgb_sum_host, g.worker->d_image, 3 * (size_t)m * sizeof(float), hipMemcpyDeviceToHost, g.stream));
  return pt_ctx_sync(&g);
}
int pt_stage_render_list(const int32_t* list, int m, int iter_first, int iter_count, float* rgb_sum_host) {
  return stage_render_list("pt_stage_render_list", list, m, m, iter_first, iter_count, rgb_sum_host);
}
// ... on a worker planned for `capacity` pixels, kept across calls while the capacity is equal
int pt_stage_render_list_capacity(const int32_t* list, int m, int capacity, int iter_first, int iter_count, float* rgb_sum_host) {
  return stage_render_list("pt_stage_render_list_capacity", list, m, capacity, iter_first, iter_count, rgb_sum_host);
}

}  // extern "C"
