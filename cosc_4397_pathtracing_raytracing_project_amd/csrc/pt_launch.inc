// pt_launch.inc — kernel selection, residency queries and launch wrappers behind ptk::KernelApi (LDS sizes: pt_lds.h).
// Included by pt_kernels.hip inside ptk::<arith>::(anonymous), after every kernel.
// ───────────────────────────── launch wrappers ─────────────────────────────
// One selector per kernel family: hands `f` the kernel instance that runs `sc` and the dynamic LDS it needs (pt_lds.h).  The
// occupancy queries and the launches both go through it — a persistent grid is only right when both name the same
// instance with the same byte count.
template <bool EX, typename F>
void with_intersect_of(const SceneTables& sc, bool legacy, F&& f) {
  const bool in_lds = tables_in_lds(sc);
  if (legacy) in_lds ? f(k_intersect_legacy<true, EX>, legacy_lds<true>(sc).total) : f(k_intersect_legacy<false, EX>, legacy_lds<false>(sc).total);
  else in_lds ? f(k_intersect<true, EX>, intersect_lds<true>(sc).total) : f(k_intersect<false, EX>, intersect_lds<false>(sc).total);
}
// exact: the rays are primary rays (depth 0), traced with the reference's exact arithmetic in every mode
template <typename F>
void with_intersect(const SceneTables& sc, bool legacy, bool exact, F&& f) {
  exact ? with_intersect_of<kD0>(sc, legacy, f) : with_intersect_of<false>(sc, legacy, f);
}
// The stage form of the grid walk; primary: the depth-0 form (k_primary's walk), else the bounce form (k_paths<kGrid>'s)
template <typename F>
void with_intersect_grid(const SceneTables& sc, bool primary, F&& f) {
  primary ? f(k_intersect_grid<kD0>, intersect_grid_lds<kFast, kD0>(sc).total) : f(k_intersect_grid<false>, intersect_grid_lds<kFast, false>(sc).total);
}
static_assert((int)kLdsTables == kSearchLdsTables, "pt_sched.h batch_form names the LDS-table search form");
// The LDS-table kernel variants assume that every leaf is a top-list entry (no subtrees).
bool leaves_fit_top(const SceneTables& sc) { return (sc.num_nodes + 1) / 2 <= kMaxTop; }
// k_features: k_intersect's LDS map; scenes whose tables stay in memory and whose leaves do not all fit the top list take the
// packet scan (every ray of a group starts at the camera), the others the top list
template <typename F>
void with_features(const SceneTables& sc, F&& f) {
  if (tables_in_lds(sc)) return f(k_features<true, false>, intersect_lds<true>(sc).total);
  if (leaves_fit_top(sc)) return f(k_features<false, false>, intersect_lds<false>(sc).total);
  return f(k_features<false, true>, intersect_lds<false>(sc).total);
}
// share: the shared loop form (one trace per chunk and run of iterations, pt_sched.h) — both forms use the same LDS map;
// split (shared form only): BatchInfo::split_records — 0, kSplitRecords or (the LDS-table form only) kFirstBounce
template <Search S, typename F>
void with_primary_of(const SceneTables& sc, bool share, int split, F&& f) {
  const int lds = primary_lds<S, kFast, kD0>(sc).total;
  if constexpr (S == kLdsTables)
    if (share && split == kFirstBounce) return f(k_primary<S, true, kFirstBounce>, lds);
  return !share ? f(k_primary<S>, lds) : split ? f(k_primary<S, true, kSplitRecords>, lds) : f(k_primary<S, true>, lds);
}
template <typename F>
void with_primary(const SceneTables& sc, bool share, int split, F&& f) {
  switch (search_form(sc)) {
    case kLdsTables: return with_primary_of<kLdsTables>(sc, share, split, f);
    case kTopScan: return with_primary_of<kTopScan>(sc, share, split, f);
    case kGrid: return with_primary_of<kGrid>(sc, share, split, f);
  }
}

// split: pt_sched.h paths_split (0, kSplitRecords; kLdsTables also kFirstBounce and kFixedSlots) — the same LDS map
template <typename F>
void with_paths(const SceneTables& sc, Search form, int split, F&& f) {  // (SceneTables::scan_nodes_lds resolved by the caller)
  switch (form) {
    case kLdsTables:
      if (split == kFirstBounce) return f(k_paths<kLdsTables, kFirstBounce>, paths_lds<kLdsTables, kFast>(sc).total);
      if (split == kFixedSlots) return f(k_paths<kLdsTables, kFixedSlots>, paths_lds<kLdsTables, kFast>(sc).total);
      return split ? f(k_paths<kLdsTables, kSplitRecords>, paths_lds<kLdsTables, kFast>(sc).total) : f(k_paths<kLdsTables>, paths_lds<kLdsTables, kFast>(sc).total);
    case kTopScan: return split ? f(k_paths<kTopScan, kSplitRecords>, paths_lds<kTopScan, kFast>(sc).total) : f(k_paths<kTopScan>, paths_lds<kTopScan, kFast>(sc).total);
    case kGrid: return split ? f(k_paths<kGrid, kSplitRecords>, paths_lds<kGrid, kFast>(sc).total) : f(k_paths<kGrid>, paths_lds<kGrid, kFast>(sc).total);
  }
}
int paths_lds_bytes(const SceneTables& sc, Search form) {
  int bytes = 0;
  with_paths(sc, form, 0, [&](auto, int lds) { bytes = lds; });
  return bytes;
}
int lds_share_limit(int bytes);
// SceneTables::scan_nodes_lds == -1 resolved: the nodes go to LDS when the scan form's workgroups per CU (LDS share) stay the same
SceneTables resolve_scan_nodes(const SceneTables& sc_in) {
  SceneTables sc = sc_in;
  // ... and k_paths' table of the RNG's per-(depth, iteration) hash factors (depth - 1 rows of max_batch_iters words; small tiles
  // run ~100-200 iterations per batch): kept while it costs no resident workgroup per CU, else the factor is hashed per ray
  // (~18 VALU per shaded ray against a sixth of the waves).
  if (iter_hash_entries(sc) > 0) {
    SceneTables without = sc;
    without.max_batch_iters = kIterHashMax + 1;
    const Search form = search_form(sc);
    const int reg_waves = form == kLdsTables ? kPathsWaves : form == kTopScan ? kPathsScanWaves : kPathsGridWaves;
    SceneTables a = sc, b = without;
    if (a.scan_nodes_lds < 0) a.scan_nodes_lds = b.scan_nodes_lds = 0;
    const bool costs = min(lds_share_limit(paths_lds_bytes(b, form)), reg_waves) > min(lds_share_limit(paths_lds_bytes(a, form)), reg_waves);
    if (costs) sc = without;
  }
  SceneTables t = sc;
  if (t.scan_nodes_lds >= 0) return t;
  SceneTables with = sc, without = sc;
  with.scan_nodes_lds = 1, without.scan_nodes_lds = 0;
  const int bw = paths_lds_bytes(with, kTopScan), bo = paths_lds_bytes(without, kTopScan);
  t.scan_nodes_lds = (bw <= 64 * 1024 && lds_share_limit(bw) >= min(lds_share_limit(bo), kPathsScanWaves)) ? 1 : 0;  // (registers allow kPathsScanWaves workgroups per CU)
  return t;
}
// Resident workgroups per CU by the runtime's count, for a selector's callback; `fallback` when the query fails.
auto occupancy_into(int& n, int fallback) {
  return [&n, fallback](auto kernel, int lds) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, kBlock, lds) != hipSuccess) n = fallback;
  };
}
// Stage the scene tables in LDS only if every leaf is a top-list entry and staging does not cost the dominant kernel
// (k_paths) a resident block per CU against its form with the tables in memory.
int lds_table_limit(const SceneTables& sc, int forced_bytes) {
  if (forced_bytes >= 0) return leaves_fit_top(sc) ? forced_bytes : -1;
  const int tbl = table_bytes(sc);
  int with = 0, without = 0;
  if (tbl <= kLdsTableBytes && leaves_fit_top(sc)) {
    SceneTables in = sc;
    in.lds_table_bytes = tbl;
    with_paths(in, kLdsTables, 0, occupancy_into(with, 0));
  }
  with_paths(sc, kTopScan, 0, occupancy_into(without, 1));
  (void)hipGetLastError();
  return (with >= without && with > 0) ? tbl : -1;
}

// The occupancy query over-reports by one workgroup when the LDS of a block is a few hundred bytes under a 1/n share of the
// CU's 160 KB (measured, round 4: 27,088 B per block: 6 reported, 5 resident — and a persistent grid one block too large runs
// that block's whole share after everybody else: k_paths 1335 -> 1607 us).  A share is therefore counted in 1280-byte granules.
constexpr int kLdsGranule = 1280;
int lds_share_limit(int bytes) { return bytes > 0 ? (160 * 1024) / (((bytes + kLdsGranule - 1) / kLdsGranule) * kLdsGranule) : 8; }
int resident_blocks_per_cu(KernelId id, const SceneTables& sc) {
  int n = 0, m = 0, lds = 0;  // lds: the fused kernels' blocks are also held to their granule share of the CU's LDS
  const auto query = occupancy_into(n, 1);
  const auto query_share = [&](auto kernel, int bytes) { query(kernel, bytes), lds = bytes; };
  switch (id) {
    case kGenerate: query(k_generate, 0); break;
    case kIntersect: with_intersect(sc, false, false, query); break;
    case kIntersectLegacy: with_intersect(sc, true, false, query); break;
    case kPrimary: with_primary(sc, false, 0, query_share); break;
    // (a context's batches run any record form of these two, BatchInfo::split_records: same LDS; the smallest count serves all — where a
    // form does not exist for the tables' search form, kFirstBounce and kFixedSlots, the selectors give the split form again)
    case kPrimaryShared:
      for (int form : kRecordForms) with_primary(sc, true, form, query_share), m = form ? min(m, n) : n;
      n = m;
      break;
    case kPaths:
      for (int form : kPathsSplits) with_paths(resolve_scan_nodes(sc), search_form(sc), form, query_share), m = form ? min(m, n) : n;
      n = m;
      if (search_form(sc) == kLdsTables) query_share(k_paths<kLdsTables, kFixedSlots, PrevGather>, paths_lds<kLdsTables, kFast>(resolve_scan_nodes(sc)).total), n = min(m, n);
      break;
    case kShade: query(k_shade, shade_lds<true>(sc).total); break;
    case kFeatures: with_features(sc, query); break;
  }
  if (n < 1) n = 1;
  n = min(n, max(1, lds_share_limit(lds)));
  return n > 8 ? 8 : n;
}

void launch_generate(hipStream_t s, int grid, const ptd::Camera& cam, const BatchInfo& b, const ptd::Queues& qs,
                     ptd::PathBuf out, int32_t* cnt0) {
  hipLaunchKernelGGL(k_generate, dim3(grid), dim3(kBlock), 0, s, cam, b, qs, out, cnt0);
}

void launch_intersect(hipStream_t s, int grid, const SceneTables& sc, const ptd::Queues& qs, const int32_t* cnt_in,
                      ptd::PathBuf paths, ptd::HitBuf hits, bool legacy, bool exact_arith) {
  with_intersect(sc, legacy, exact_arith, [&](auto kernel, int lds) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, s, sc, qs, cnt_in, paths, hits); });
}

void launch_intersect_grid(hipStream_t s, int grid, const SceneTables& sc, const ptd::Queues& qs, const int32_t* cnt_in,
                           ptd::PathBuf paths, ptd::HitBuf hits, bool primary) {
  with_intersect_grid(sc, primary, [&](auto kernel, int lds) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, s, sc, qs, cnt_in, paths, hits); });
}

void launch_primary(hipStream_t s, int grid, const SceneTables& sc, const ptd::Camera& cam, const BatchInfo& b,
                    const ptd::Queues& qs, int32_t* cnt0, int32_t* cnt_out, ptd::PathBuf out, ptd::RetireBuf ret) {
  with_primary(sc, primary_shares(b), b.split_records, [&](auto kernel, int lds) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, s, sc, cam, b, qs, cnt0, cnt_out, out, ret); });
}

void launch_features(hipStream_t s, int grid, const SceneTables& sc, const ptd::Camera& cam, const BatchInfo& b, float4* feat) {
  with_features(sc, [&](auto kernel, int lds) {
    // tables of up to kLdsTableBytes plus the waves' blocks: above the 64 KB a kernel gets without asking
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, s, sc, cam, b, feat);
  });
}

void launch_paths(hipStream_t s, int grid, const SceneTables& sc_in, const BatchInfo& b, const ptd::Queues& qs, int32_t* cnt, ptd::PathBuf in, ptd::RetireBuf ret) {
  const SceneTables sc = resolve_scan_nodes(sc_in);
  with_paths(sc, search_form(sc), paths_split(b.split_records, b.fixed_slots != 0), [&](auto kernel, int lds) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, s, sc, b, qs, cnt, in, ret); });
}
// The fixed-slot instance that also gathers the previous batch (k_paths, PREV): the LDS-table form only, the same LDS map
void launch_paths_gather(hipStream_t s, int grid, const SceneTables& sc_in, const BatchInfo& b, const ptd::Queues& qs, int32_t* cnt, ptd::PathBuf in,
                         ptd::RetireBuf ret, const PrevGather& prev) {
  const SceneTables sc = resolve_scan_nodes(sc_in);
  const auto kernel = k_paths<kLdsTables, kFixedSlots, PrevGather>;
  const int lds = paths_lds<kLdsTables, kFast>(sc).total;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, s, sc, b, qs, cnt, in, ret, prev);
}
void launch_shade(hipStream_t s, int grid, const SceneTables& sc, const BatchInfo& b, int depth, const ptd::Queues& qs,
                  const int32_t* cnt_in, int32_t* cnt_out, ptd::PathBuf in, ptd::HitBuf hits, ptd::PathBuf out,
                  ptd::RetireBuf ret) {
  hipLaunchKernelGGL(k_shade, dim3(grid), dim3(kBlock), shade_lds<true>(sc).total, s, sc, b, depth, qs, cnt_in, cnt_out, in, hits, out,
                     ret);
}

int flat_grid(int n, int cap) {
  int grid = (n + kBlock - 1) / kBlock;
  return grid > cap ? cap : (grid < 1 ? 1 : grid);
}
void launch_collect(hipStream_t s, const BatchInfo& b, const ptd::Queues& qs, ptd::RetireBuf ret, float* image_rgb) {
  // 96 KB of dynamic LDS (and the residues' retiree counts): above the 64 KB a kernel gets without asking (per device: set on every launch, it is cheap)
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_collect), hipFuncAttributeMaxDynamicSharedMemorySize, collect_lds_bytes(ret.wq0));
  hipLaunchKernelGGL(k_collect, dim3(qs.Q), dim3(kCollectThreads), collect_lds_bytes(ret.wq0), s, b, qs, ret, image_rgb);
}
// The stream gather and the counter rows in one launch: ceil(seg_cap / kBlock) blocks per queue, then k_count_stats' depth_count + 2
void launch_collect_stream(hipStream_t s, const BatchInfo& b, const ptd::Queues& qs, ptd::RetireBuf ret, float* image_rgb, int32_t* cnt, int depth_count,
                           unsigned long long* stats) {
  const int per_queue = (ret.seg_cap + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_collect_stream, dim3(qs.Q * per_queue + depth_count + 2), dim3(kBlock), 0, s, b, qs, ret, image_rgb, per_queue, cnt, depth_count, stats);
}
void launch_collect_stream_planes(hipStream_t s, const BatchInfo& b, const ptd::Queues& qs, ptd::RetireBuf ret, const ptd::Word4* plane0, float* image_rgb) {
  const int per_queue = (ret.seg_cap + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_collect_stream_planes, dim3(qs.Q * per_queue), dim3(kBlock), 0, s, b, qs, ret, plane0, image_rgb, per_queue);
}
void launch_collect_conv(hipStream_t s, const BatchInfo& b, const ptd::Queues& qs, ptd::RetireBuf ret, float* image_rgb, const ConvInfo& cv, double* sse) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_collect_conv), hipFuncAttributeMaxDynamicSharedMemorySize, collect_lds_bytes(ret.wq0));
  hipLaunchKernelGGL(k_collect_conv, dim3(qs.Q), dim3(kCollectThreads), collect_lds_bytes(ret.wq0), s, b, qs, ret, image_rgb, cv);
  if (cv.first_k < b.K) hipLaunchKernelGGL(k_conv_reduce, dim3(b.K - cv.first_k), dim3(kBlock), 0, s, b.iter_first, cv.first_k, qs.Q * kCollectWaves, cv.partial, sse);
}

#include "pt_ieee_check.inc"
#include "pt_fast_math_check.inc"

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
  hipLaunchKernelGGL(k_shade_stage, dim3(flat_grid(n, 2048)), dim3(kBlock), shade_lds<false>(sc).total, s, sc, trace_depth, depth, n, iter, pixel, hits,
                     paths, alive);
}
