// pt_launch.inc — LDS sizing, residency queries and launch wrappers behind ptk::KernelApi.
// Included by pt_kernels.hip inside ptk::<arith>::(anonymous), after every kernel.
// ───────────────────────────── launch wrappers ─────────────────────────────
int fused_lds_bytes(const SceneTables& sc, bool in_lds, int wave_lds, bool primary = false) {
  int bytes = sc.num_top * (int)sizeof(ptd::TopEntry) + round16(sc.num_mats * (int)sizeof(ptd::Mat)) + kWavesPerBlock * wave_lds + iter_hash_entries(sc) * 4;
  if (in_lds) bytes += round16(sc.num_nodes * (int)sizeof(ptd::Node) + sc.num_geoms * (int)sizeof(ptd::Geom));
  if (primary) bytes += sc.num_top * (int)sizeof(ptd::TopEntry) + (in_lds ? round16(sc.num_geoms * 12) : 0);  // camera-relative copies
  return bytes;
}
int table_bytes(const SceneTables& sc) { return sc.num_nodes * (int)sizeof(ptd::Node) + sc.num_geoms * (int)sizeof(ptd::Geom); }
bool tables_in_lds(const SceneTables& sc) { return table_bytes(sc) <= sc.lds_table_bytes; }
// k_paths' search form: 2 = uniform grid walk, 0 = scene tables in LDS (every leaf a top entry), 1 = top list + subtree scans
int paths_mode(const SceneTables& sc) { return sc.use_grid ? 2 : (tables_in_lds(sc) ? 0 : 1); }
int lds_share_limit(int bytes);
int paths_lds_bytes(const SceneTables& sc, int mode);
// SceneTables::scan_nodes_lds == -1 resolved: the nodes go to LDS when the scan form's workgroups per CU (LDS share) stay the same
SceneTables resolve_scan_nodes(const SceneTables& sc_in) {
  SceneTables sc = sc_in;
  // ... and k_paths' table of the RNG's per-(depth, iteration) hash factors (depth - 1 rows of max_batch_iters words; small tiles
  // run ~100-200 iterations per batch): kept while it costs no resident workgroup per CU, else the factor is hashed per ray
  // (~18 VALU per shaded ray against a sixth of the waves).
  if (iter_hash_entries(sc) > 0) {
    SceneTables without = sc;
    without.max_batch_iters = kIterHashMax + 1;
    const int mode = paths_mode(sc);
    const int reg_waves = mode == 0 ? kPathsWaves : mode == 1 ? kPathsScanWaves : kPathsGridWaves;
    SceneTables a = sc, b = without;
    if (a.scan_nodes_lds < 0) a.scan_nodes_lds = b.scan_nodes_lds = 0;
    const bool costs = min(lds_share_limit(paths_lds_bytes(b, mode)), reg_waves) > min(lds_share_limit(paths_lds_bytes(a, mode)), reg_waves);
    if (costs) sc = without;
  }
  SceneTables t = sc;
  if (t.scan_nodes_lds >= 0) return t;
  SceneTables with = sc, without = sc;
  with.scan_nodes_lds = 1, without.scan_nodes_lds = 0;
  const int bw = paths_lds_bytes(with, 1), bo = paths_lds_bytes(without, 1);
  t.scan_nodes_lds = (bw <= 64 * 1024 && lds_share_limit(bw) >= min(lds_share_limit(bo), kPathsScanWaves)) ? 1 : 0;  // (registers allow kPathsScanWaves workgroups per CU)
  return t;
}
int paths_lds_bytes(const SceneTables& sc, int mode) {
  const int rows = iter_hash_entries(sc) * 4 * max(0, sc.trace_depth - 1), common = round16(sc.num_mats * (int)sizeof(ptd::Mat)) + rows;
  const int top = sc.num_top * (int)sizeof(ptd::TopEntry);
  switch (mode) {
    case 0: return common + top + sc.num_geoms * (int)sizeof(ptd::Geom) + kWavesPerBlock * paths_wave_bytes<0>() + kMaxTop * 4 + 64 * 4;
    case 1: return common + top + kWavesPerBlock * paths_wave_bytes<1>() + (sc.scan_nodes_lds > 0 ? sc.num_nodes * (int)sizeof(ptd::Node) : 0);
    default: return common + kWavesPerBlock * paths_wave_bytes<2>();
  }
}
int primary_grid_lds_bytes(const SceneTables& sc) {
  return round16(sc.num_mats * (int)sizeof(ptd::Mat)) + kWavesPerBlock * grid_wave_bytes<kD0>() + iter_hash_entries(sc) * 4;
}
// The LDS-table kernel variants assume that every leaf is a top-list entry (no subtrees).
bool leaves_fit_top(const SceneTables& sc) { return (sc.num_nodes + 1) / 2 <= kMaxTop; }
// Stage the scene tables in LDS only if every leaf is a top-list entry and staging does not cost the dominant kernel
// (k_paths) a resident block per CU against its form with the tables in memory.
int lds_table_limit(const SceneTables& sc, int forced_bytes) {
  if (forced_bytes >= 0) return leaves_fit_top(sc) ? forced_bytes : -1;
  const int tbl = table_bytes(sc);
  int with = 0, without = 0;
  if (tbl <= kLdsTableBytes && leaves_fit_top(sc)) {
    SceneTables in = sc;
    in.lds_table_bytes = tbl;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&with, k_paths<0>, kBlock, paths_lds_bytes(in, 0)) != hipSuccess) with = 0;
  }
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&without, k_paths<1>, kBlock, paths_lds_bytes(sc, 1)) != hipSuccess) without = 1;
  (void)hipGetLastError();
  return (with >= without && with > 0) ? tbl : -1;
}

// The occupancy query over-reports by one workgroup when the LDS of a block is a few hundred bytes under a 1/n share of the
// CU's 160 KB (measured, round 4: 27,088 B per block: 6 reported, 5 resident — and a persistent grid one block too large runs
// that block's whole share after everybody else: k_paths 1335 -> 1607 us).  A share is therefore counted in 1280-byte granules.
constexpr int kLdsGranule = 1280;
int lds_share_limit(int bytes) { return bytes > 0 ? (160 * 1024) / (((bytes + kLdsGranule - 1) / kLdsGranule) * kLdsGranule) : 8; }
int resident_blocks_per_cu(KernelId id, const SceneTables& sc) {
  int n = 0, lds = 0;
  hipError_t e = hipSuccess;
  const int tbl = table_bytes(sc);
  const bool in_lds = tables_in_lds(sc);
  switch (id) {
    case kGenerate:
      e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_generate, kBlock, 0);
      break;
    case kIntersect:
      if (in_lds)
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_intersect<true, false>, kBlock, round16(tbl) + kWavesPerBlock * kWaveLds + sc.num_top * (int)sizeof(ptd::TopEntry));
      else
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_intersect<false, false>, kBlock, kWavesPerBlock * kWaveLds + sc.num_top * (int)sizeof(ptd::TopEntry));
      break;
    case kIntersectLegacy:
      if (in_lds) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_intersect_legacy<true, false>, kBlock, round16(tbl));
      else e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_intersect_legacy<false, false>, kBlock, 0);
      break;
    case kPrimary:
      if (sc.use_grid) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_primary<false, true>, kBlock, lds = primary_grid_lds_bytes(sc));
      else if (in_lds) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_primary<true>, kBlock, lds = fused_lds_bytes(sc, true, carry_bytes<true>(), true));
      else e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_primary<false>, kBlock, lds = fused_lds_bytes(sc, false, kWaveLds, true));
      break;
    case kPaths:
      lds = paths_lds_bytes(resolve_scan_nodes(sc), paths_mode(sc));
      if (paths_mode(sc) == 0) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_paths<0>, kBlock, lds);
      else if (paths_mode(sc) == 1) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_paths<1>, kBlock, lds);
      else e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_paths<2>, kBlock, lds);
      break;
    case kShade:
      e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_shade, kBlock, round16(sc.num_mats * (int)sizeof(ptd::Mat)) + iter_hash_entries(sc) * 4);
      break;
  }
  if (e != hipSuccess || n < 1) n = 1;
  n = min(n, max(1, lds_share_limit(lds)));
  return n > 8 ? 8 : n;
}

void launch_generate(hipStream_t s, int grid, const ptd::Camera& cam, const BatchInfo& b, const ptd::Queues& qs,
                     ptd::PathBuf out, int32_t* cnt0) {
  hipLaunchKernelGGL(k_generate, dim3(grid), dim3(kBlock), 0, s, cam, b, qs, out, cnt0);
}

// exact_arith: the rays are primary rays (depth 0), traced with the reference's exact arithmetic in every mode
void launch_intersect(hipStream_t s, int grid, const SceneTables& sc, const ptd::Queues& qs, const int32_t* cnt_in,
                      ptd::PathBuf paths, ptd::HitBuf hits, bool legacy, bool exact_arith) {
  const int bytes = table_bytes(sc);
  const bool in_lds = tables_in_lds(sc);
  const bool ex = kD0 && exact_arith;
  const int wave_lds = kWavesPerBlock * kWaveLds + sc.num_top * (int)sizeof(ptd::TopEntry);
  const int lds = legacy ? (in_lds ? round16(bytes) : 0) : (in_lds ? round16(bytes) : 0) + wave_lds;
#define PT_LAUNCH_ISECT(K) hipLaunchKernelGGL(K, dim3(grid), dim3(kBlock), lds, s, sc, qs, cnt_in, paths, hits)
  if (legacy) {
    if (in_lds) { if (ex) PT_LAUNCH_ISECT((k_intersect_legacy<true, kD0>)); else PT_LAUNCH_ISECT((k_intersect_legacy<true, false>)); }
    else { if (ex) PT_LAUNCH_ISECT((k_intersect_legacy<false, kD0>)); else PT_LAUNCH_ISECT((k_intersect_legacy<false, false>)); }
  } else {
    if (in_lds) { if (ex) PT_LAUNCH_ISECT((k_intersect<true, kD0>)); else PT_LAUNCH_ISECT((k_intersect<true, false>)); }
    else { if (ex) PT_LAUNCH_ISECT((k_intersect<false, kD0>)); else PT_LAUNCH_ISECT((k_intersect<false, false>)); }
  }
#undef PT_LAUNCH_ISECT
}

void launch_primary(hipStream_t s, int grid, const SceneTables& sc, const ptd::Camera& cam, const BatchInfo& b,
                    const ptd::Queues& qs, int32_t* cnt0, int32_t* cnt_out, ptd::PathBuf out, ptd::RetireBuf ret) {
  if (sc.use_grid) hipLaunchKernelGGL((k_primary<false, true>), dim3(grid), dim3(kBlock), primary_grid_lds_bytes(sc), s, sc, cam, b, qs, cnt0, cnt_out, out, ret);
  else if (tables_in_lds(sc)) hipLaunchKernelGGL(k_primary<true>, dim3(grid), dim3(kBlock), fused_lds_bytes(sc, true, carry_bytes<true>(), true), s, sc, cam, b, qs, cnt0, cnt_out, out, ret);
  else hipLaunchKernelGGL(k_primary<false>, dim3(grid), dim3(kBlock), fused_lds_bytes(sc, false, kWaveLds, true), s, sc, cam, b, qs, cnt0, cnt_out, out, ret);
}

void launch_paths(hipStream_t s, int grid, const SceneTables& sc_in, const BatchInfo& b, const ptd::Queues& qs, int32_t* cnt, ptd::PathBuf in, ptd::RetireBuf ret) {
  const SceneTables sc = resolve_scan_nodes(sc_in);
  const int bytes = paths_lds_bytes(sc, paths_mode(sc));
  if (paths_mode(sc) == 0) hipLaunchKernelGGL(k_paths<0>, dim3(grid), dim3(kBlock), bytes, s, sc, b, qs, cnt, in, ret);
  else if (paths_mode(sc) == 1) hipLaunchKernelGGL(k_paths<1>, dim3(grid), dim3(kBlock), bytes, s, sc, b, qs, cnt, in, ret);
  else hipLaunchKernelGGL(k_paths<2>, dim3(grid), dim3(kBlock), bytes, s, sc, b, qs, cnt, in, ret);
}
void launch_shade(hipStream_t s, int grid, const SceneTables& sc, const BatchInfo& b, int depth, const ptd::Queues& qs,
                  const int32_t* cnt_in, int32_t* cnt_out, ptd::PathBuf in, ptd::HitBuf hits, ptd::PathBuf out,
                  ptd::RetireBuf ret) {
  const int bytes = round16(sc.num_mats * (int)sizeof(ptd::Mat)) + iter_hash_entries(sc) * 4;
  hipLaunchKernelGGL(k_shade, dim3(grid), dim3(kBlock), bytes, s, sc, b, depth, qs, cnt_in, cnt_out, in, hits, out,
                     ret);
}

int flat_grid(int n, int cap) {
  int grid = (n + kBlock - 1) / kBlock;
  return grid > cap ? cap : (grid < 1 ? 1 : grid);
}
void launch_collect(hipStream_t s, const BatchInfo& b, const ptd::Queues& qs, ptd::RetireBuf ret, float* image_rgb) {
  // 96 KB of dynamic LDS: above the 64 KB a kernel gets without asking (per device: set on every launch, it is cheap)
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_collect), hipFuncAttributeMaxDynamicSharedMemorySize, collect_lds_bytes());
  hipLaunchKernelGGL(k_collect, dim3(qs.Q), dim3(kCollectThreads), collect_lds_bytes(), s, b, qs, ret, image_rgb);
}
void launch_collect_conv(hipStream_t s, const BatchInfo& b, const ptd::Queues& qs, ptd::RetireBuf ret, float* image_rgb, const ConvInfo& cv, double* sse) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_collect_conv), hipFuncAttributeMaxDynamicSharedMemorySize, collect_lds_bytes());
  hipLaunchKernelGGL(k_collect_conv, dim3(qs.Q), dim3(kCollectThreads), collect_lds_bytes(), s, b, qs, ret, image_rgb, cv);
  if (cv.first_k < b.K) hipLaunchKernelGGL(k_conv_reduce, dim3(b.K - cv.first_k), dim3(kBlock), 0, s, b.iter_first, cv.first_k, qs.Q * kCollectWaves, cv.partial, sse);
}

#include "pt_ieee_check.inc"

void launch_count_stats(hipStream_t s, const ptd::Queues& qs, int32_t* cnt, int depth_count,
                        unsigned long long* stats) {
  hipLaunchKernelGGL(k_count_stats, dim3(depth_count + 2), dim3(kBlock), 0, s, qs, cnt, depth_count, stats);  // + the block that deals k_paths' waves
}

void launch_preview(hipStream_t s, int n, int iterations, const float* image_rgb, uchar4* rgba) {
  hipLaunchKernelGGL(k_preview, dim3(flat_grid(n, 4096)), dim3(kBlock), 0, s, n, iterations, image_rgb, rgba);
}

void launch_save_u8(hipStream_t s, int n, int width, float samples, const float* image_rgb, uint8_t* rgb8) {
  hipLaunchKernelGGL(k_save_u8, dim3(flat_grid(n, 4096)), dim3(kBlock), 0, s, n, width, samples, image_rgb, rgb8);
}

void launch_shade_stage(hipStream_t s, const SceneTables& sc, int trace_depth, int depth, int n, const int32_t* iter,
                        const int32_t* pixel, ptd::HitBuf hits, ptd::PathBuf paths, int32_t* alive) {
  const int bytes = round16(sc.num_mats * (int)sizeof(ptd::Mat));
  hipLaunchKernelGGL(k_shade_stage, dim3(flat_grid(n, 2048)), dim3(kBlock), bytes, s, sc, trace_depth, depth, n, iter, pixel, hits,
                     paths, alive);
}
