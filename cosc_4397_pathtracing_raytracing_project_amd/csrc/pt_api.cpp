// pt_api.cpp — C ABI (include/pt_amd.h) and device-state owner of the MI355X
// wavefront path tracer.  Host C++ calling the HIP runtime directly; replaces the
// reference's pathtraceInit / pathtrace / pathtraceFree (src/pathtrace.cu:446-653).
// Here: the error state, a context's lifecycle, run_batch, readback, the scene functions and the single-instance API; pt_post.cpp is
// what reads or extends a rendered image, pt_stage.cpp the tests' stages, pt_context.h the context and the helpers the three share.
//
// Differences from the reference's host loop by design:
//   * no host<->device synchronisation inside an iteration (the reference does ~38),
//     no per-iteration malloc/free, no per-iteration D2H frame copies or printf;
//   * K iterations are traced as one wavefront batch so each launch has enough rays;
//   * kernel sizes are fixed (persistent grid), live counts stay on the device.
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "pt_adaptive.h"
#include "pt_camera_tables_device.h"
#include "pt_context.h"
#include "pt_lds.h"
#include "pt_scene.h"
#include "pt_sched.h"

namespace {

std::string g_err;
constexpr int kDebugFlags = 16 | 32 | 64 | 256 | 512 | 2048 | ptk::kFormSwitches;  // the PtOptions.debug_flags bits pt_init accepts
static_assert(sizeof(PtOptions) == 80, "capi.PtOptions mirrors this layout");
static_assert(PT_CONVERGENCE_WAVES == ptk::kConvWaves, "pt_amd.h documents the size of the convergence metric's partial sums");
}  // namespace
int pt_fail(const char* fmt, ...) {  // pt_internal.h: sets pt_last_error(), returns -1
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return -1;
}

namespace ptc {
static PtContext* g_default = nullptr;
PtContext* default_context() { return g_default; }

int get_events(Ctx& g, EventPair* ev) {
  if (!g.free_events.empty()) {
    *ev = g.free_events.back();
    g.free_events.pop_back();
    return 0;
  }
  HIP_OK(hipEventCreate(&ev->a));
  HIP_OK(hipEventCreate(&ev->b));
  return 0;
}
static int resolve_events(Ctx& g) {  // requires the stream to be idle
  auto drain = [&](std::vector<EventPair>& pending, double& total_ms) -> int {
    for (auto& e : pending) {
      float ms = 0;
      HIP_OK(hipEventElapsedTime(&ms, e.a, e.b));
      total_ms += ms;
      g.free_events.push_back(e);
    }
    pending.clear();
    return 0;
  };
  g.isect_launches += (int64_t)g.pending_isect.size();
  return drain(g.pending_isect, g.isect_ms) || drain(g.pending_render, g.render_ms) ? -1 : 0;
}

ptk::SceneTables tables(const Ctx& g) {
  ptk::SceneTables t = g.scene;
  if (g.debug_flags & 16) t.cull_margin = INFINITY;
  if (g.debug_flags & 32) t.top_xor = 0;
  t.lds_table_bytes = g.lds_table_bytes;
  t.max_batch_iters = g.K;
  t.trace_depth = g.depth;
  t.scan_nodes_lds = -1;  // resolved per kernel (pt_launch.inc resolve_scan_nodes)
  // debug_flags 256 builds and uses the grid for any scene, 512 never (A/B, same results)
  t.use_grid = !g.grids.empty() && g.grid_enabled && !(g.debug_flags & 512) ? 1 : 0;
  if (t.use_grid) {
    const Ctx::DeviceGrid& gr = g.grids[g.grid_pick];
    t.lds_table_bytes = -1;  // (a forced grid on a small scene: the grid kernels read the tables from memory)
    t.grid_start = gr.d_start + gr.guard;
    t.grid_items = gr.d_items;
    t.grid_items_b = gr.d_items_b;
    for (int a = 0; a < 3; ++a)
      t.grid_res[a] = gr.shape.res[a], t.grid_min[a] = gr.shape.gmin[a], t.grid_cs[a] = gr.shape.cs[a], t.grid_inv_cs[a] = gr.shape.inv_cs[a];
    t.grid_pad = gr.shape.pad;
  }
  return t;
}

static size_t pathbuf_words(int64_t stride) { return (size_t)(2 * stride + (stride * ptd::kPathPlane2Bytes + 15) / 16); }
static int alloc_pathbuf(Ctx& g, ptd::PathBuf* b, int64_t stride) {
  b->stride = stride;
  // planes 0 and 1: 16 bytes per path, plane 2: kPathPlane2Bytes (pt_device.h); allocated in 16-byte words
  return dalloc(g, &b->r, pathbuf_words(stride));
}
static int alloc_hitbuf(Ctx& g, ptd::HitBuf* h, int64_t stride) {
  h->stride = stride;
  return dalloc(g, &h->t, stride) || dalloc(g, &h->n, 3 * stride) || dalloc(g, &h->mat, stride) || dalloc(g, &h->p, 3 * stride) ? -1 : 0;
}

// Queue descriptor for a launch of `grid` workgroups (W = waves of THAT launch; Q, cap shared).
static ptd::Queues queues_for(const Ctx& g, int grid) {
  ptd::Queues q = g.qs;
  q.W = grid * ptk::kWavesPerBlock;
  return q;
}

// BatchInfo::primary_share of the context's batches: debug_flags kTraceEveryIteration and a primary_share of 1 both mean a trace per
// iteration; automatic: the longest run, a whole piece per trace (on the whole frame caps of 8 to 64 iterations measure alike, 4 is
// 0.5 % slower: profiles/first_hit_sharing.log section 2b).
static int primary_share_of(const Ctx& g) { return (g.debug_flags & ptk::kTraceEveryIteration) ? 1 : g.primary_share ? g.primary_share : ptk::kShareMax; }

ptk::BatchInfo tile_batch(const Ctx& g, int iter_first, int K) {
  ptk::BatchInfo b{};
  b.iter_first = iter_first;
  b.K = K;
  b.N = g.N;
  b.pixel_begin = g.pixel_begin;
  b.trace_depth = g.depth;
  b.aa_jitter = g.aa_jitter ? 1 : 0;
  b.stripe = g.stripe;
  b.gap = g.stripe ? g.stripe_stride - g.stripe : 0;
  b.inv_stripe = g.stripe ? 1.0f / (float)g.stripe : 0.0f;
  return b;
}
// ... and the fields pt_sched.h batch_form reads besides, in every batch of the context (the unfused kernels' batches are flat: whole records)
static ptk::BatchInfo form_batch(const Ctx& g, int iter_first, int K) {
  ptk::BatchInfo b = tile_batch(g, iter_first, K);
  b.slot_shift = g.slot_shift, b.flat = g.fuse_bounces ? 0 : 1, b.primary_share = primary_share_of(g);
  return b;
}

// The stream gather of the batch that waits (pt_sched.h gather_plan) as a launch of its own: its successor could not take it.
static void gather_waiting(Ctx& g) {
  if (!g.waiting.live) return;
  ptd::RetireBuf ret = g.ret;
  if (g.waiting.plane) ret.rec = g.rec_plane1;
  g.k->collect_stream_planes(g.stream, g.waiting.b, g.qs, ret, g.ret.rec, g.d_image);
  g.waiting.live = false;
}

int run_batch(Ctx& g, int iter_first, int kb, int after) {
  // 1. the batch
  ptk::BatchInfo b = form_batch(g, iter_first, kb);
  b.paths_pieces = g.paths_pieces, b.list = g.list;
  if (b.list) b.stripe = 1, b.gap = 0, b.inv_stripe = 1.0f;  // (BatchInfo::list: the list form sits behind the stripe test)
  const ptk::SceneTables sc = tables(g);
  // 2. its form (pt_sched.h batch_form), decided once, handed to the kernels here
  const ptk::BatchForm form = ptk::batch_form(ptk::form_inputs(b, g.debug_flags, ptk::search_form(sc), sc.num_mats, g.ret.seg_cap));
  b.retire_once = form.retire_once, b.split_records = g.record_form = form.records, b.fixed_slots = form.fixed_slots;
  b.primary_pieces = form.shares ? ptk::auto_shared_pieces(kb, g.qs.nq, g.ret.wq0) : ptk::auto_primary_pieces(kb, g.qs.nq, g.ret.wq0);
  if (g.primary_pieces) b.primary_pieces = g.primary_pieces;
  if (form.records == ptk::kFirstBounce) b.primary_pieces = 1;  // one trace per chunk and batch: primary_pieces / primary_share cut nothing
  const ptk::KernelApi& k = *g.k;
  auto cnt_row = [&](int d) { return g.d_cnt + ptk::cnt_index(g.qs, d, 0); };  // the counter row of depth d
  // 3. depth 0 once per camera (BatchForm::primary_once; never without k_primary: flat): do an earlier batch's first-hit records serve this
  // one?  Until this batch is submitted whole they serve nobody (a batch of another form overwrites them, a failed one leaves them undefined).
  const ptd::Queues pq = queues_for(g, g.grid_primary);
  Ctx::PrimaryKey key;
  std::memset(&key, 0, sizeof(key));
  key.sc = sc, key.cam = g.dcam, key.b = b, key.b.iter_first = key.b.K = 0, key.qs = pq, key.out = g.buf[1], key.ret = g.ret;
  key.kernels = &k, key.grid = g.grid_primary, key.debug_flags = g.debug_flags;
  const bool same_key = form.primary_once && g.primary_valid && std::memcmp(&key, &g.primary_key, sizeof(key)) == 0;
  g.primary_valid = false;
  // 4. the gather (pt_sched.h gather_plan)
  ptk::ConvInfo cv{g.d_ref, g.d_partial, -1, kb};
  if (g.conv_live) {
    if (g.conv_have_ref) cv.first_k = 0;
    else if (g.conv >= iter_first && g.conv < iter_first + kb) cv.capture_k = g.conv - iter_first, cv.first_k = cv.capture_k + 1, g.conv_have_ref = true;
    g.conv_last = std::max(g.conv_last, iter_first + kb - 1);
  }
  const bool all_depths = g.grid_paths > 0;  // depths >= 1 fused
  const ptk::GatherPlan plan = ptk::gather_plan({form, cv.capture_k >= 0 || cv.first_k < kb, g.waiting.live, g.waiting.plane, same_key,
                                                 g.rec_plane1 != nullptr && !g.conv, after, g.debug_flags, all_depths});
  ptd::RetireBuf ret = g.ret;
  if (plan.plane) ret.rec = g.rec_plane1;
  // 5. the launches
  if (!plan.gathers_waiting) gather_waiting(g);  // before k_primary rewrites what that gather reads
  if (!g.fuse_primary) k.generate(g.stream, g.grid_gen, g.dcam, b, queues_for(g, g.grid_gen), g.buf[0], cnt_row(0));
  else if (!same_key) {
    // depth 0 in one launch; its survivors are the depth-1 input (buf[1], cnt[1])
    k.primary(g.stream, g.grid_primary, sc, g.dcam, b, pq, cnt_row(0), cnt_row(1), g.buf[1], g.ret);
    g.primary_launches += 1;
    std::memcpy(&g.primary_key, &key, sizeof(key));
  }
  const int d0 = g.fuse_primary ? 1 : 0;
  int src = d0;
  // Depths >= 1, fused: ONE launch of k_paths — persistent lanes with their own depth, no path state through HBM after depth 0
  EventPair ev{};  // brackets the dominant kernel of a depth (fused: of all depths) when the context times its kernels
  auto timed_from = [&]() -> int {
    if (!g.time_kernels) return 0;
    if (get_events(g, &ev)) return -1;
    HIP_OK(hipEventRecord(ev.a, g.stream));
    return 0;
  };
  auto timed_to = [&]() -> int {
    if (!g.time_kernels) return 0;
    HIP_OK(hipEventRecord(ev.b, g.stream));
    g.pending_isect.push_back(ev);
    return 0;
  };
  if (all_depths) {
    if (timed_from()) return -1;
    if (plan.gathers_waiting) {
      const ptk::PrevGather prev{g.waiting.plane ? g.rec_plane1 : g.ret.rec, g.ret.rec, g.d_image, g.waiting.b.K, 0};
      k.paths_gather(g.stream, g.grid_paths, sc, b, queues_for(g, g.grid_paths), g.d_cnt, g.buf[1], ret, prev);
      g.waiting.live = false;
      g.inline_gathers += 1;
    } else k.paths(g.stream, g.grid_paths, sc, b, queues_for(g, g.grid_paths), g.d_cnt, g.buf[1], ret);
    if (timed_to()) return -1;
  }
  // ... unfused (tests, A/B): computeIntersections and shadeAndExtendRays as separate launches per depth
  for (int d = d0; d < g.depth && !all_depths; ++d) {
    const int32_t* cin = cnt_row(d);
    int32_t* cout = cnt_row(d + 1);
    if (timed_from()) return -1;
    k.intersect(g.stream, g.grid_isect, sc, queues_for(g, g.grid_isect), cin, g.buf[src], g.hits, g.legacy, d == 0);
    if (timed_to()) return -1;
    k.shade(g.stream, g.grid_shade, sc, b, d, queues_for(g, g.grid_shade), cin, cout, g.buf[src], g.hits, g.buf[src ^ 1], g.ret);
    src ^= 1;
  }
  // The closing launch (pt_sched.h Closing).  A batch whose gather waits for its successor's k_paths folds only the counter rows now.
  g.gather_form = plan.reported;
  if (plan.closing == ptk::kCloseStream) k.collect_stream(g.stream, b, g.qs, g.ret, g.d_image, g.d_cnt, g.depth, g.d_stats);
  else k.count_stats(g.stream, g.qs, g.d_cnt, g.depth, g.d_stats);
  if (plan.closing == ptk::kCloseStatsStreamPlanes) k.collect_stream_planes(g.stream, b, g.qs, ret, g.ret.rec, g.d_image);
  if (plan.closing == ptk::kCloseStatsConv) k.collect_conv(g.stream, b, g.qs, g.ret, g.d_image, cv, g.d_sse);
  if (plan.closing == ptk::kCloseStatsTile) k.collect(g.stream, b, g.qs, g.ret, g.d_image);
  if (plan.defers) g.waiting.live = true, g.waiting.b = b, g.waiting.plane = plan.plane;
  HIP_OK(hipGetLastError());
  g.primary_valid = form.primary_once;
  g.samples += (int64_t)kb * g.N;
  if (g.pending_isect.size() > 16384) {
    HIP_OK(hipStreamSynchronize(g.stream));
    if (resolve_events(g)) return -1;
  }
  return 0;
}

// Launch geometry (persistent grids = resident workgroups) for the kernels the current tables select.
void plan_launch(Ctx& g) {
  if (!g.borrowed) g.lds_table_bytes = g.k->lds_table_limit(tables(g), g.lds_table_forced);  // (a worker keeps its parent's decision)
  const ptk::SceneTables t = tables(g);
  g.grid_gen = g.num_cus * std::min(g.cap_bpc, g.k->resident_blocks_per_cu(ptk::kGenerate, t));
  g.grid_isect = g.num_cus * std::min(g.cap_bpc, g.k->resident_blocks_per_cu(g.legacy ? ptk::kIntersectLegacy : ptk::kIntersect, t));
  g.grid_shade = g.num_cus * std::min(g.cap_bpc, g.k->resident_blocks_per_cu(ptk::kShade, t));
  g.grid_primary = g.num_cus * std::min(g.cap_bpc, g.k->resident_blocks_per_cu(ptk::primary_shares(form_batch(g, 0, g.K)) ? ptk::kPrimaryShared : ptk::kPrimary, t));
  g.ret.wq0 = ptk::wave_slot(0, g.qs.Q, g.grid_primary * ptk::kWavesPerBlock).wq;  // the sub-lists' residue count (pt_device.h RetireBuf)
  g.grid_paths = (g.fuse_bounces && g.depth > 1) ? g.num_cus * std::min(g.cap_bpc, g.k->resident_blocks_per_cu(ptk::kPaths, t)) : 0;
  g.qs.paths_W = g.grid_paths * ptk::kWavesPerBlock;  // what k_count_stats deals to the queues (a table made for another width is ignored)
  g.primary_valid = false;  // (the first-hit records of another plan: pt_sched.h BatchForm::primary_once)
}

// A grid's device memory back to the device (choose_traversal's losers, a camera move that changes a grid's size).
static void free_grid(Ctx& g, const Ctx::DeviceGrid& d) {
  for (void* p : {(void*)d.d_start, (void*)d.d_items, d.d_items_b != d.d_items ? (void*)d.d_items_b : nullptr}) {
    if (!p) continue;
    (void)hipFree(p);
    g.allocs.erase(std::remove(g.allocs.begin(), g.allocs.end(), p), g.allocs.end());
  }
  g.device_bytes -= (int64_t)d.bytes;
}
// Grid or BVH scan, and which grid?  All give the same image (LABNOTES.md section 9.1); which is faster depends on how the
// primitives are spread and how far rays fly, and no count of references predicted it across lattice, random and clustered
// scenes — so it is measured: up to 8 iterations of the context's own tile with each (the second of two runs counts), before
// the first sample is rendered.  Costs a few tens of milliseconds per candidate for a 1080p tile.  debug_flags 256 / 512 skip
// the measurement.
static int choose_traversal(Ctx& g) {
  auto drop_unused_grids = [&](size_t keep) {
    for (size_t i = 0; i < g.grids.size(); ++i)
      if (i != keep) free_grid(g, g.grids[i]);
    g.grids = {g.grids[keep]};
    g.grid_pick = 0;
  };
  if (g.grids.empty()) return 0;
  if (!g.fuse_bounces || (g.debug_flags & (256 | 512))) {
    drop_unused_grids(0);
    return 0;
  }
  auto time_one = [&](float* ms) -> int {
    plan_launch(g);
    for (int rep = 0; rep < 2; ++rep) {
      EventPair ev{};
      if (get_events(g, &ev)) return -1;
      HIP_OK(hipEventRecord(ev.a, g.stream));
      if (run_batch(g, 1, std::min(g.K, 8))) return -1;  // enough groups per wave for the persistent grids to fill
      HIP_OK(hipEventRecord(ev.b, g.stream));
      HIP_OK(hipStreamSynchronize(g.stream));
      HIP_OK(hipEventElapsedTime(ms, ev.a, ev.b));
      g.free_events.push_back(ev);
    }
    return 0;
  };
  g.grid_enabled = false;
  if (time_one(&g.probe_ms[0])) return -1;
  g.grid_enabled = true;
  size_t best = 0;
  for (size_t i = 0; i < g.grids.size(); ++i) {
    float ms = 0.f;
    g.grid_pick = i;
    if (time_one(&ms)) return -1;
    // a finer grid has to beat the model's by 3 %, so that the choice does not flip between runs on timing noise
    if (i == 0 || ms < 0.97f * g.probe_ms[1]) g.probe_ms[1] = ms, best = i;
  }
  drop_unused_grids(best);
  // the grid has to win by a margin: two short timed runs on a shared or noisy box differ by a few per cent, and a
  // choice that flips between runs makes PtStats and profiles irreproducible; results are equal either way
  g.grid_enabled = g.probe_ms[1] < 0.95f * g.probe_ms[0];
  plan_launch(g);
  HIP_OK(hipMemsetAsync(g.d_image, 0, 3 * (size_t)g.N * sizeof(float), g.stream));
  HIP_OK(hipMemsetAsync(g.d_stats, 0, PT_MAX_DEPTH * sizeof(unsigned long long), g.stream));
  HIP_OK(hipStreamSynchronize(g.stream));
  g.samples = 0;
  g.primary_launches = 0;
  return 0;
}

ptd::Queues single_queue(const Ctx& g, int n) {
  ptd::Queues qs{};
  qs.Q = 1;
  const ptk::QueuePlan p = ptk::queue_plan(n, 1, 1);
  qs.cap = p.cap;
  qs.W = g.grid * ptk::kWavesPerBlock;
  qs.cnt_stride = 16;
  qs.nq = p.nq;
  qs.inv_nq = 1.0f / (float)qs.nq;
  return qs;
}

void destroy(Ctx* c) {
  if (!c) return;
  destroy(c->worker);
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (void* p : c->allocs) (void)hipFree(p);
  auto kill = [](std::vector<EventPair>& v) {
    for (auto& e : v) {
      (void)hipEventDestroy(e.a);
      (void)hipEventDestroy(e.b);
    }
    v.clear();
  };
  kill(c->free_events);
  kill(c->pending_isect);
  kill(c->pending_render);
  if (c->stream && !c->borrowed) (void)hipStreamDestroy(c->stream);
  delete c;
}

// The device, its stream and the kernels of the arithmetic mode.
static int open_device(Ctx& g, const PtOptions& opt) {
  g.arith = opt.arith;
  g.k = ptk::api_for(opt.arith);
  if (!g.k) return pt_fail("pt_init: arith %d is not one of PT_ARITH_EXACT / PT_ARITH_FMA / PT_ARITH_FAST", opt.arith);
  if (opt.convergence < -1) return pt_fail("pt_init: convergence %d is not 0 (off), N > 0 (frame captured at iteration N) or -1 (frame supplied)", opt.convergence);
  if (opt.convergence > PT_CONVERGENCE_CAPACITY) return pt_fail("pt_init: convergence %d exceeds PT_CONVERGENCE_CAPACITY (%d iterations)", opt.convergence, PT_CONVERGENCE_CAPACITY);
  if (opt.primary_pieces > 0 && (opt.primary_pieces >> 16) > ptk::kShareMax) return pt_fail("pt_init: primary_pieces 0x%x: primary_share %d exceeds %d (PT_PRIMARY_PIECES)", opt.primary_pieces, opt.primary_pieces >> 16, ptk::kShareMax);
  if (opt.debug_flags & ~kDebugFlags) return pt_fail("pt_init: debug_flags 0x%x: bits 0x%x are not defined", opt.debug_flags, opt.debug_flags & ~kDebugFlags);
  int ndev = 0;
  HIP_OK(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return pt_fail("pt_init: no HIP device (this library has no CPU fallback)");
  if (opt.device < 0 || opt.device >= ndev) return pt_fail("pt_init: device %d of %d", opt.device, ndev);
  g.device = opt.device;
  HIP_OK(hipSetDevice(g.device));
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, g.device));
  g.num_cus = prop.multiProcessorCount;
  HIP_OK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
  return 0;
}

// The camera, the scene's sizes and the options that choose kernels and schedules.
static void take_camera(PtShared& g, const PtCamera& cam) {
  g.cam = cam;
  g.dcam.res_x = g.cam.resolution[0], g.dcam.res_y = g.cam.resolution[1];
  std::memcpy(g.dcam.pos, g.cam.position, 12);
  std::memcpy(g.dcam.view, g.cam.view, 12);
  std::memcpy(g.dcam.up, g.cam.up, 12);
  std::memcpy(g.dcam.right, g.cam.right, 12);
  g.dcam.pl_x = g.cam.pixelLength[0], g.dcam.pl_y = g.cam.pixelLength[1];
}
static void take_scene_and_options(Ctx& g, const PtSceneDesc* sc, const PtOptions& opt) {
  take_camera(g, sc->camera);
  g.depth = sc->trace_depth;
  g.legacy = opt.legacy_traversal != 0;
  g.aa_jitter = opt.aa_jitter != 0;
  g.debug_flags = opt.debug_flags;
  g.conv = opt.convergence;
  auto pieces = [](int v, int automatic) { return v ? std::clamp(v, 1, 0x7fff) : automatic; };
  g.lds_table_forced = opt.lds_table_kb ? std::clamp(opt.lds_table_kb, 0, ptk::kLdsTableBytes / 1024) * 1024 : -1;
  g.primary_pieces = pieces(opt.primary_pieces < 0 ? opt.primary_pieces : opt.primary_pieces & 0xffff, 0);
  g.primary_share = opt.primary_pieces < 0 ? 0 : std::min(opt.primary_pieces >> 16 & 0x7f, ptk::kShareMax);  // PT_PRIMARY_PIECES
  g.paths_pieces = ptk::pack_paths_pieces(pieces(opt.paths_pieces, 2), pieces(opt.paths_min_piece, 64));
  g.fuse_primary = !g.legacy && !opt.unfused_primary;
  g.fuse_bounces = g.fuse_primary && !opt.unfused_bounces;
  g.cap_bpc = opt.blocks_per_cu > 0 ? std::min(opt.blocks_per_cu, 8) : 8;
}

// Iterations per batch of a tile of N pixels (iters_per_batch <= 0: automatic) and its BatchInfo::slot_shift; -1 after a failure.
// One function for a context's own plan and for what a worker of pt_render_adaptive WOULD plan before it exists.
int batch_iters_for(int iters_per_batch, int N, int* slot_shift) {
  // batch size: enough paths in flight to fill the chip a few times over; slots are int32
  int K = iters_per_batch;
  if (K <= 0) {
    const int64_t target = 48ll << 20;  // ~50 M paths per batch (24 iterations of 1920x1080, ~5 GB of path state):
                                        // launch boundaries drop below 1 % of a batch (measured K=6 → 48: +8 %)
    K = (int)std::max<int64_t>(1, std::min<int64_t>(256, (target + N - 1) / N));
  }
  // sample ids are k << slot_shift | tile pixel in 31 bits (BatchInfo::slot_shift)
  int shift = 1;
  while ((1ll << shift) < N) ++shift;
  if (shift > 30) return pt_fail("pt_init: tiles of more than 2^30 pixels are not supported");
  while (K > 1 && K > (1 << (31 - shift))) --K;
  if (slot_shift) *slot_shift = shift;
  return K;
}

// The tile, the iterations per batch and the compaction queues.
int plan_batches(Ctx& g, const PtOptions& opt) {
  const int W = g.cam.resolution[0], H = g.cam.resolution[1];
  g.opt_iters_per_batch = opt.iters_per_batch, g.opt_num_queues = opt.num_queues;
  g.pixel_begin = opt.pixel_begin;
  g.N = opt.pixel_count > 0 ? opt.pixel_count : W * H - opt.pixel_begin;
  g.stripe = opt.stripe_pixels;
  g.stripe_stride = opt.stripe_stride;
  if (g.stripe < 0 || (g.stripe > 0 && g.stripe_stride < g.stripe)) return pt_fail("pt_init: bad stripe %d / stride %d", g.stripe, g.stripe_stride);
  {
    // last global pixel the tile touches
    int64_t last = (int64_t)g.pixel_begin + g.N - 1;
    if (g.stripe > 0) last = (int64_t)g.pixel_begin + (g.N - 1) + (int64_t)((g.N - 1) / g.stripe) * (g.stripe_stride - g.stripe);
    if (g.pixel_begin < 0 || g.N <= 0 || last >= (int64_t)W * H)
      return pt_fail("pt_init: tile [%d, +%d, stripe %d/%d) outside %dx%d", opt.pixel_begin, opt.pixel_count, g.stripe, g.stripe_stride, W, H);
    if (g.stripe > 0 && g.N / g.stripe >= 32768) return pt_fail("pt_init: more than 32767 stripes");
    if (H >= 32768) return pt_fail("pt_init: image height %d not supported (>= 32768)", H);
  }
  const int K = batch_iters_for(opt.iters_per_batch, g.N, &g.slot_shift);
  if (K < 0) return -1;

  // Compaction queues: every launch needs (waves % Q) == 0, so Q divides 4 * CUs.  A queue owns every Q-th 64-pixel
  // chunk of the tile in every iteration (pt_device.h); k_collect wants at most 128 chunks per queue (one LDS tile per
  // pass), so large tiles get more queues while the waves allow it.
  int Q = opt.num_queues > 0 ? opt.num_queues : 256;
  const int cu_waves = g.num_cus * ptk::kWavesPerBlock;
  if (Q > cu_waves) Q = cu_waves;
  while (cu_waves % Q) --Q;
  if (opt.num_queues <= 0)
    while (ptk::chunks_per_queue(g.N, Q) > 128 && 2 * Q <= cu_waves && cu_waves % (2 * Q) == 0) Q *= 2;
  const ptk::QueuePlan plan = ptk::queue_plan(g.N, Q, K);
  const int grid = g.num_cus * 8;
  // Retirement records: one slot per (iteration of the batch, pixel) — regions (queue, iteration) of nq * 64 slots, exactly
  // full at the end of a batch (pt_device.h RetireBuf): 16 bytes per sample and batch.
  g.K = K;
  g.grid = grid;
  g.qs.Q = Q;
  g.qs.W = grid * ptk::kWavesPerBlock;
  g.qs.cnt_stride = 16;
  g.qs.nq = plan.nq;
  g.qs.inv_nq = 1.0f / (float)plan.nq;
  g.qs.cap = plan.cap;
  g.stride = (int64_t)Q * g.qs.cap;
  g.ret.seg_cap = plan.seg_cap;
  g.ret.kmax = K;
  return 0;
}

// A device copy of `v`; nullptr after a failure.
template <typename T>
static const T* upload(Ctx& g, const std::vector<T>& v) {
  T* p = nullptr;
  if (dalloc(g, &p, v.size())) return nullptr;
  const hipError_t e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return e == hipSuccess ? p : (pt_fail("hipMemcpy(%zu bytes) failed: %s", v.size() * sizeof(T), hipGetErrorString(e)), nullptr);
}
static int upload_grid(Ctx& g, const pt::Grid& gr) {  // one more entry of g.grids
  Ctx::DeviceGrid d{gr.shape, gr.guard, nullptr, nullptr, nullptr, 0, gr.start};
  const int64_t before = g.device_bytes;
  if (!(d.d_start = upload(g, gr.start)) || !(d.d_items = upload(g, gr.items))) return -1;
  if (!(d.d_items_b = gr.items_b.empty() ? d.d_items : upload(g, gr.items_b))) return -1;
  d.bytes = (size_t)(g.device_bytes - before);
  d.items = gr.items.size();
  g.grids.push_back(d);
  return 0;
}
// What pt::build_scene_tables built, on the device (g.scene), the grids as candidates for choose_traversal().
static int upload_tables(Ctx& g, const pt::HostTables& t) {
  ptk::SceneTables& s = g.scene;
  s.num_nodes = (int)t.nodes.size(), s.num_geoms = (int)t.geoms.size(), s.num_mats = (int)t.mats.size(), s.num_top = (int)t.top.size();
  std::memcpy(s.root_min, t.root_min, 12);
  std::memcpy(s.root_max, t.root_max, 12);
  s.cull_margin = t.cull_margin;
  s.top_xor = t.top_xor;
  s.has_triangles = t.has_triangles ? 1 : 0;
  g.tight_leaves = t.tight_leaves;
  if (!(s.nodes = upload(g, t.nodes)) || !(s.geoms = upload(g, t.geoms)) || !(s.mats = upload(g, t.mats)) || !(s.top = upload(g, t.top))) return -1;
  s.nodes_b = s.nodes, s.top_b = s.top;  // the bounce kernels' box tables: the same, except for the fast build's centre / half extent copies
  if (!t.nodes_b.empty() && (!(s.nodes_b = upload(g, t.nodes_b)) || !(s.top_b = upload(g, t.top_b)))) return -1;
  for (const pt::Grid& gr : t.grids)
    if (upload_grid(g, gr)) return -1;
  return 0;
}

// Every retirement record slot := (quiet NaN, NaN, NaN, tile pixel chunk_pixel(q, 0, Q) of the slot's queue q); see alloc_batch_buffers.
static __global__ void k_poison_records(ptd::Word4* rec, unsigned long long per_queue, unsigned long long total, int Q) {
  const float nan = __builtin_nanf("");
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * blockDim.x)
    rec[i] = ptd::Word4{nan, nan, nan, __int_as_float(ptk::chunk_pixel((int)(i / per_queue), 0, Q))};
}

static int poison_records(Ctx& g) {  // on the context's stream; the plan in g.ret must be the one the records were allocated for
  const size_t regions = (size_t)g.qs.Q * g.ret.kmax, per_queue = (size_t)g.ret.kmax * g.ret.seg_cap;
  for (ptd::Word4* plane : {g.ret.rec, g.rec_plane1})
    if (plane)
      hipLaunchKernelGGL(k_poison_records, dim3((unsigned)std::min<size_t>((regions * g.ret.seg_cap + 255) / 256, 65536)), dim3(256), 0, g.stream, plane,
                         (unsigned long long)per_queue, (unsigned long long)(regions * g.ret.seg_cap), g.qs.Q);
  HIP_OK(hipGetLastError());
  return 0;
}
static size_t sub_words_max(const Ctx& g) { return ptk::sub_stride(g.num_cus * 8 * ptk::kWavesPerBlock, g.qs.Q); }  // (8 resident workgroups per CU at the most)

// The "first batch of a context" state of alloc_batch_buffers again, on the stream, for a context that starts over with another view
// (pt_ctx_set_camera): path buffers all ones, records poisoned, fill levels and the deal of the waves zero.  A slot wrongly gathered
// from the previous view then shows as NaN, not as a plausible pixel.
static int rearm_batch_buffers(Ctx& g) {
  g.primary_valid = false;  // the first-hit records go with the buffers (pt_sched.h batch_form)
  for (const ptd::PathBuf& pb : g.buf) HIP_OK(hipMemsetAsync(pb.r, 0xff, pathbuf_words(pb.stride) * sizeof(ptd::Word4), g.stream));
  const size_t regions = (size_t)g.qs.Q * g.ret.kmax;
  HIP_OK(hipMemsetAsync(g.ret.cnt, 0, regions * sizeof(*g.ret.cnt), g.stream));
  HIP_OK(hipMemsetAsync(g.ret.sub, 0, regions * sub_words_max(g) * sizeof(*g.ret.sub), g.stream));
  if (g.qs.deal) HIP_OK(hipMemsetAsync(g.qs.deal, 0, (size_t)ptk::deal_map(g.qs).words() * sizeof(int32_t), g.stream));
  return poison_records(g);
}

// Path state, hit records, retirement records, image, counters.
int alloc_batch_buffers(Ctx& g) {
  const int Q = g.qs.Q;
  if (alloc_pathbuf(g, &g.buf[0], g.stride) || alloc_pathbuf(g, &g.buf[1], g.stride)) return -1;
  // In a BatchInfo::split_records batch the invariant half of a depth-1 record is written by ONE run of k_primary and read in every
  // iteration; a later batch finds an older batch's identical words there.  So the path buffers start as NaN (all bits set) in every
  // word, like the retirement records below: a slot nobody wrote in this batch then shows in the first batch of a context.
  for (const ptd::PathBuf& pb : g.buf) HIP_OK(hipMemset(pb.r, 0xff, pathbuf_words(pb.stride) * sizeof(ptd::Word4)));
  if (!g.fuse_bounces && alloc_hitbuf(g, &g.hits, g.stride)) return -1;  // hit records reach HBM only in the unfused form
  {
    const size_t regions = (size_t)Q * g.ret.kmax;
    const size_t wq_max = sub_words_max(g);
    if (dalloc(g, &g.ret.rec, regions * g.ret.seg_cap)) return -1;
    // The second record plane (pt_sched.h gather_plan), where a context's batches can be of that form at all: the fused kernels and no
    // switch against it (kNoSecondPlane); whether a batch has fixed slots is decided per batch.  A failed allocation leaves the context on
    // the standalone gather.  (A context with the convergence metric gets the plane too — PtStats.device_bytes differs by the metric's own
    // buffers, as documented — and never uses it; a worker's batches are single launches of run_batch: none.)
    g.rec_plane1 = nullptr;
    if (g.fuse_primary && g.fuse_bounces && g.depth > 1 && !g.aa_jitter && !g.borrowed && !(g.debug_flags & ptk::kNoSecondPlane)) {
      void* p = nullptr;
      const size_t bytes = regions * g.ret.seg_cap * sizeof(ptd::Word4);
      if (hipMalloc(&p, bytes) == hipSuccess) {
        g.allocs.push_back(p);
        g.device_bytes += (int64_t)bytes;
        g.rec_plane1 = static_cast<ptd::Word4*>(p);
      } else (void)hipGetLastError();
    }
    // the fill levels start at zero; k_collect re-zeroes them after every batch
    if (ensure(g, g.ret.cnt, regions * sizeof(*g.ret.cnt), Zero::blocking) || ensure(g, g.ret.sub, regions * wq_max * sizeof(*g.ret.sub), Zero::blocking)) return -1;
    // In a BatchInfo::retire_once batch nobody writes the retiree slots at the front of the regions k >= 1, and later they hold an older
    // batch's identical records: a gather that wrongly read them would still produce the right image.  So every slot starts as
    // (NaN, NaN, NaN, first pixel of the slot's queue) — a wrongly gathered slot then shows in the first batch of a context.
    if (poison_records(g)) return -1;
  }
  const size_t image_bytes = 3 * (size_t)g.N * sizeof(float);
  const size_t cnt_words = ptk::cnt_index(g.qs, g.depth + 1, 0);  // rows 0 .. depth; k_count_stats re-zeroes them after every batch
  if (ensure(g, g.d_image, image_bytes, Zero::blocking) || ensure(g, g.d_cnt, cnt_words * sizeof(int32_t), Zero::blocking) ||
      ensure(g, g.d_stats, PT_MAX_DEPTH * sizeof(*g.d_stats), Zero::blocking))
    return -1;
  // (debug_flags 64: W / Q waves per queue in every batch; same image)  zero: nothing measured yet, W / Q each
  if (!(g.debug_flags & 64) && ensure(g, g.qs.deal, (size_t)ptk::deal_map(g.qs).words() * sizeof(int32_t), Zero::blocking)) return -1;
  if (g.conv) {
    const size_t partials = (size_t)g.K * Q * ptk::kConvWaves;  // zero: queues without pixels never write theirs
    if (ensure(g, g.d_ref, image_bytes, Zero::blocking) || ensure(g, g.d_partial, partials * sizeof(double), Zero::blocking)) return -1;
    if (dalloc(g, &g.d_sse, (size_t)PT_CONVERGENCE_CAPACITY)) return -1;
    HIP_OK(hipMemset(g.d_sse, 0xff, (size_t)PT_CONVERGENCE_CAPACITY * sizeof(double)));
  }
  HIP_OK(hipDeviceSynchronize());
  return 0;
}

// pathtraceInit (pathtrace.cu:462-516) for one context.  Any failure leaves nothing behind: the caller destroys `g`.
static int setup(Ctx& g, const PtSceneDesc* sc, const PtOptions& opt) {
  if (open_device(g, opt)) return -1;
  take_scene_and_options(g, sc, opt);
  if (plan_batches(g, opt)) return -1;
  if ((size_t)sc->num_materials * sizeof(ptd::Mat) > 60 * 1024) return pt_fail("pt_init: %zu materials exceed the LDS table", (size_t)sc->num_materials);
  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
  clock::time_point t0 = clock::now();
  const pt::HostTables host = pt::build_scene_tables(*sc, g.debug_flags, g.k->boxes_center_half != 0, pt::GridRequest{}, &g.camera_base);
  g.setup_times.tables_ms = ms_since(t0), t0 = clock::now();
  if (upload_tables(g, host)) return -1;
  g.materials.assign(sc->materials, sc->materials + sc->num_materials);
  g.setup_times.upload_ms = ms_since(t0), t0 = clock::now();
  plan_launch(g);
  if (alloc_batch_buffers(g)) return -1;
  g.setup_times.buffers_ms = ms_since(t0), t0 = clock::now();
  if (choose_traversal(g)) return -1;
  g.setup_times.probe_ms = ms_since(t0);
  // what a camera move rebuilds (pt_ctx_set_camera): the grid the kernels walk, at its resolution, or none
  g.grid_request.kind = pt::GridRequest::kNone;
  if (tables(g).use_grid) {
    g.grid_request.kind = pt::GridRequest::kFixed;
    std::memcpy(g.grid_request.res, g.grids[g.grid_pick].shape.res, sizeof(g.grid_request.res));
  }
  g.time_kernels = opt.time_kernels != 0;
  g.conv_live = g.conv != 0;
  return 0;
}

int need(const PtContext* c, const char* who) { return c ? 0 : pt_fail("%s: pt_init has not been called", who); }

int admit(const PtContext& g, const char* who, unsigned req) {
  if ((req & kNotFailed) && g.failed) return pt_fail("%s: an earlier batch of this context failed (%s); free it and create a new one", who, g_err.c_str());
  // what reads the image as "SUM over one number of samples" has no meaning once pixels differ in their sample counts
  if ((req & kUniform) && g.adaptive)
    return pt_fail("%s: the renderer is in the adaptive state (pt_adaptive_round): one sample count no longer describes the image; read it with pt_resolve, or "
                   "return to the uniform state with pt_clear", who);
  if ((req & kNoExtras) && g.hist_extra)
    return pt_fail("%s: the history round left extra samples in some pixels (pt_history_round): one sample count no longer describes the image; read it with "
                   "pt_history_resolve, or return to the uniform state with pt_clear", who);
  const int W = g.cam.resolution[0];
  if ((req & kWholeRows) && (g.stripe || g.pixel_begin % W || g.N % W))
    return pt_fail("%s: the tile must consist of whole contiguous image rows (begin %d, count %d, stripe %d, width %d)", who, g.pixel_begin, g.N, g.stripe, W);
  if ((req & kFoldedAll) && g.rendered != g.noise_iters)
    return pt_fail("%s: %lld iteration(s) rendered since the last fold; fold first (pt_noise_fold)", who, (long long)(g.rendered - g.noise_iters));
  if (req & kOnDevice) HIP_OK(hipSetDevice(g.device));
  return 0;
}

}  // namespace ptc
using namespace ptc;

extern "C" {

const char* pt_last_error(void) { return g_err.c_str(); }

int pt_selfcheck_ieee(int arith, int kind, uint64_t first, uint64_t count, uint32_t seed, uint64_t* mismatches) {
  const ptk::KernelApi* k = ptk::api_for(arith);
  if (!k || kind < 0 || kind > 4 || !mismatches) return pt_fail("pt_selfcheck_ieee: bad argument");
  unsigned long long* d = nullptr;
  HIP_OK(hipMalloc(&d, sizeof(*d)));
  hipError_t e = hipMemset(d, 0, sizeof(*d));
  if (e == hipSuccess) {
    k->ieee_check(nullptr, kind, first, count, seed, d);
    e = hipGetLastError();
  }
  unsigned long long h = 0;
  if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return pt_fail("pt_selfcheck_ieee: %s", hipGetErrorString(e));
  *mismatches = h;
  return 0;
}

int pt_selfcheck_fast_math(int arith, int kind, uint64_t first, uint64_t count, double* max_err) {
  const ptk::KernelApi* k = ptk::api_for(arith);
  if (!k || kind < 0 || kind > 8 || !max_err) return pt_fail("pt_selfcheck_fast_math: bad argument");
  unsigned long long* d = nullptr;
  HIP_OK(hipMalloc(&d, sizeof(*d)));
  hipError_t e = hipMemset(d, 0, sizeof(*d));
  if (e == hipSuccess) {
    k->fast_math_check(nullptr, kind, first, count, d);
    e = hipGetLastError();
  }
  unsigned long long h = 0;
  if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return pt_fail("pt_selfcheck_fast_math: %s", hipGetErrorString(e));
  std::memcpy(max_err, &h, sizeof(h));  // the bits of a non-negative double
  return 0;
}

// ---- scene -----------------------------------------------------------------
struct PtScene {
  pt::Scene scene;
  explicit PtScene(const std::string& f) : scene(f) {}
};

int pt_scene_load(const char* path, int res_w, int res_h, PtScene** out) {
  if (!path || !out) return pt_fail("pt_scene_load: null argument");
  try {
    PtScene* s = new PtScene(path);
    if (res_w > 0 && res_h > 0) s->scene.overrideResolution(res_w, res_h);
    s->scene.applyInitialCameraState();
    *out = s;
    return 0;
  } catch (const std::exception& e) {
    return pt_fail("pt_scene_load: %s", e.what());
  }
}
void pt_scene_free(PtScene* s) { delete s; }
int pt_scene_desc(const PtScene* s, PtSceneDesc* out) {
  if (!s || !out) return pt_fail("pt_scene_desc: null argument");
  *out = s->scene.desc();
  return 0;
}
int pt_scene_orbit(PtScene* s, float dphi, float dtheta, float dzoom) {
  if (!s) return pt_fail("pt_scene_orbit: null scene");
  s->scene.orbit(dphi, dtheta, dzoom);
  return 0;
}
int pt_scene_camera(const PtScene* s, PtCamera* out) {
  if (!s || !out) return pt_fail("pt_scene_camera: null argument");
  *out = s->scene.state.camera;
  return 0;
}
int pt_scene_orbit_state(const PtScene* s, float* phi, float* theta, float* zoom) {
  if (!s) return pt_fail("pt_scene_orbit_state: null scene");
  if (phi) *phi = s->scene.phi;
  if (theta) *theta = s->scene.theta;
  if (zoom) *zoom = s->scene.zoom;
  return 0;
}
// The geom's OBJECT placement, or the refusal under the name `who`.
static int scene_geom(const PtScene* s, int geom, const void* trs, const char* who) {
  if (!s || !trs) return pt_fail("%s: null argument", who);
  if (geom < 0 || (size_t)geom >= s->scene.geoms.size()) return pt_fail("%s: geom %d is outside the scene's %zu geoms", who, geom, s->scene.geoms.size());
  if (s->scene.geom_trs[(size_t)geom].mesh) return pt_fail("%s: geom %d is a triangle of a mesh object: its vertices are world-space, it has no TRS of its own", who, geom);
  return 0;
}
int pt_scene_geom_trs(const PtScene* s, int geom, float trs[9]) {
  if (scene_geom(s, geom, trs, "pt_scene_geom_trs")) return -1;
  std::memcpy(trs, s->scene.geom_trs[(size_t)geom].trs, 9 * sizeof(float));
  return 0;
}
int pt_scene_set_geom_trs(PtScene* s, int geom, const float trs[9]) {
  if (scene_geom(s, geom, trs, "pt_scene_set_geom_trs")) return -1;
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(trs[k])) return pt_fail("pt_scene_set_geom_trs: trs[%d] is not finite", k);
  s->scene.placeGeom(geom, trs);
  return 0;
}
// The material's slot, or the refusal under the name `who`.
static int scene_material(const PtScene* s, int m, const void* arg, const char* who) {
  if (!s || !arg) return pt_fail("%s: null argument", who);
  if (m < 0 || (size_t)m >= s->scene.materials.size()) return pt_fail("%s: material %d is outside the scene's %zu materials", who, m, s->scene.materials.size());
  return 0;
}
int pt_scene_material(const PtScene* s, int m, PtMaterial* out) {
  if (scene_material(s, m, out, "pt_scene_material")) return -1;
  *out = s->scene.materials[(size_t)m];
  return 0;
}
int pt_scene_set_material(PtScene* s, int m, const PtMaterial* material) {
  if (scene_material(s, m, material, "pt_scene_set_material")) return -1;
  if (!s->scene.setMaterial(m, *material)) return pt_fail("pt_scene_set_material: material %d has a word that is not finite", m);
  return 0;
}
int pt_scene_iterations(const PtScene* s) { return s ? (int)s->scene.state.iterations : 0; }
const char* pt_scene_image_name(const PtScene* s) { return s ? s->scene.state.imageName.c_str() : ""; }

int pt_build_bvh(const PtGeom* geoms, int num_geoms, PtBVHNode* out, int cap) {
  std::vector<PtBVHNode> nodes;
  pt::buildBVH(geoms, num_geoms, nodes);
  if (out) std::memcpy(out, nodes.data(), sizeof(PtBVHNode) * std::min<size_t>(nodes.size(), (size_t)std::max(cap, 0)));
  return (int)nodes.size();
}

int pt_traversal_boxes(const PtGeom* geoms, int num_geoms, const float camera_position[3], float* boxes) {
  if (!geoms || num_geoms <= 0 || !camera_position || !boxes) return pt_fail("pt_traversal_boxes: null argument");
  pt::ThreadedBvh bvh = pt::threaded_bvh(geoms, num_geoms);
  double olo[3], ohi[3];
  pt::origin_region(bvh.ref[0].bmin, bvh.ref[0].bmax, camera_position, olo, ohi);
  const int tightened = pt::tighten_sphere_leaves(bvh.nodes, geoms, olo, ohi);  // whatever the scene's size
  for (const ptd::Node& n : bvh.nodes)
    if (n.geom >= 0) std::memcpy(boxes + 6 * (size_t)n.geom, n.bmin, 12), std::memcpy(boxes + 6 * (size_t)n.geom + 3, n.bmax, 12);
  return tightened;
}

int pt_build_grid(const PtGeom* geoms, int num_geoms, int forced, PtGridInfo* info, uint32_t* cell_start, PtGridRecord* records) {
  if (!geoms || num_geoms <= 0 || !info) return pt_fail("pt_build_grid: null argument");
  const pt::ThreadedBvh bvh = pt::threaded_bvh(geoms, num_geoms);
  std::memset(info, 0, sizeof(*info));
  info->num_leaves = num_geoms;
  if (!forced && (int)bvh.nodes.size() < pt::kGridNodes) return 0;
  pt::Grid gr;  // the reference's leaf boxes, no camera (coord_mag 0), the cost model's resolution, no guard cells
  if (!pt::build_grid(bvh.nodes, geoms, num_geoms, bvh.ref[0].bmin, bvh.ref[0].bmax, 0.0, 0.0, forced != 0, gr)) return 0;
  for (int a = 0; a < 3; ++a) info->res[a] = gr.shape.res[a], info->origin[a] = gr.shape.gmin[a], info->cell_size[a] = gr.shape.cs[a];
  info->pad = gr.shape.pad;
  info->num_cells = (int32_t)(gr.start.size() - 1);
  info->num_records = (int32_t)gr.items.size();
  if (cell_start) std::memcpy(cell_start, gr.start.data(), gr.start.size() * sizeof(uint32_t));
  static_assert(sizeof(PtGridRecord) == sizeof(ptd::Node), "PtGridRecord mirrors the device record");
  if (records) std::memcpy(records, gr.items.data(), gr.items.size() * sizeof(ptd::Node));
  return 1;
}

void pt_center_half_box(const float lo[3], const float hi[3], int inner, float magnitude, float center[3], float half_extent[3]) {
  float a[3] = {lo[0], lo[1], lo[2]}, b[3] = {hi[0], hi[1], hi[2]};
  pt::center_half_box(a, b, inner != 0, (double)magnitude);
  std::memcpy(center, a, 12);
  std::memcpy(half_extent, b, 12);
}

int pt_build_transform(const float* trs, float* transform, float* inverse, float* invTranspose) {
  if (!trs || !transform || !inverse || !invTranspose) return pt_fail("pt_build_transform: null argument");
  pt::buildTransform(trs, transform, inverse, invTranspose);
  return 0;
}

// ---- renderer contexts ---------------------------------------------------------
int pt_ctx_create(const PtSceneDesc* sc, const PtOptions* opt_in, PtContext** out) {
  if (!out) return pt_fail("pt_ctx_create: null output");
  *out = nullptr;
  if (!sc) return pt_fail("pt_init: null scene");
  if (sc->num_geoms <= 0 || !sc->geoms) return pt_fail("pt_init: scene has no geometry");
  if (sc->num_materials <= 0 || !sc->materials) return pt_fail("pt_init: scene has no materials");
  if (sc->trace_depth <= 0 || sc->trace_depth > PT_MAX_DEPTH) return pt_fail("pt_init: trace_depth %d out of range", sc->trace_depth);
  const int W = sc->camera.resolution[0], H = sc->camera.resolution[1];
  if (W <= 0 || H <= 0 || (int64_t)W * H > (1ll << 30)) return pt_fail("pt_init: bad resolution %dx%d", W, H);
  for (int i = 0; i < sc->num_geoms; ++i) {
    if (sc->geoms[i].materialid < 0 || sc->geoms[i].materialid >= sc->num_materials)
      return pt_fail("pt_init: geom %d references material %d of %d", i, sc->geoms[i].materialid, sc->num_materials);
    if (sc->geoms[i].type < PT_GEOM_SPHERE || sc->geoms[i].type > PT_GEOM_TRIANGLE)
      return pt_fail("pt_init: geom %d has unknown type %d", i, sc->geoms[i].type);
  }
  PtOptions opt{};
  if (opt_in) opt = *opt_in;
  PtContext* c = new PtContext();
  if (setup(*c, sc, opt)) {  // nothing half-initialised survives a failure
    destroy(c);
    return -1;
  }
  *out = c;
  return 0;
}

int pt_ctx_destroy(PtContext* c) {
  if (c == g_default) g_default = nullptr;
  destroy(c);
  return 0;
}

int pt_ctx_render(PtContext* c, int iter_first, int iter_count) {
  if (need(c, "pt_render")) return -1;
  if (iter_count <= 0) return 0;
  Ctx& g = *c;
  if (admit(g, "pt_render", kNotFailed | kUniform)) return -1;
  if (g.conv_live) {
    if (iter_first < 1 || (int64_t)iter_first + iter_count - 1 > PT_CONVERGENCE_CAPACITY)
      return pt_fail("pt_render: iterations %d .. %lld outside 1 .. %d (PT_CONVERGENCE_CAPACITY) with the convergence metric on", iter_first,
                  (long long)iter_first + iter_count - 1, PT_CONVERGENCE_CAPACITY);
    if (g.conv < 0 && !g.conv_have_ref) return pt_fail("pt_render: PtOptions.convergence is -1 but no reference frame has been supplied (pt_set_reference)");
  }
  HIP_OK(hipSetDevice(g.device));
  EventPair ev{};
  if (get_events(g, &ev)) return -1;
  HIP_OK(hipEventRecord(ev.a, g.stream));
  const int end = iter_first + iter_count;
  for (int it = iter_first; it < end; it += g.K)
    if (run_batch(g, it, std::min(g.K, end - it), it + g.K < end ? (end - it - 1) / g.K : 0)) {
      g.failed = true;
      g.free_events.push_back(ev);  // back to the pool (destroy() releases it)
      return -1;
    }
  HIP_OK(hipEventRecord(ev.b, g.stream));
  g.pending_render.push_back(ev);
  g.rendered += iter_count;
  g.fb_pending = false;  // the feedback's pending plane was the filter of another image
  return 0;
}

int pt_ctx_sync(PtContext* c) {
  if (need(c, "pt_sync")) return -1;
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipStreamSynchronize(c->stream));
  return resolve_events(*c);
}

int pt_ctx_readback(PtContext* c, float* out) {
  if (need(c, "pt_readback")) return -1;
  return copy_out(c, "pt_readback", out, 3, [&](const float** d) { return *d = c->d_image, 0; });
}

int pt_ctx_readback_device(PtContext* c, void* out) {
  if (need(c, "pt_readback_device")) return -1;
  return copy_out(c, "pt_readback_device", static_cast<float*>(out), 3, [&](const float** d) { return *d = c->d_image, 0; }, hipMemcpyDeviceToDevice);
}

const float* pt_ctx_device_image(PtContext* c) { return c ? c->d_image : nullptr; }
void* pt_ctx_stream(PtContext* c) { return c ? (void*)c->stream : nullptr; }
int pt_ctx_pixel_count(const PtContext* c) { return c ? c->N : 0; }
int pt_ctx_device(const PtContext* c) { return c ? c->device : -1; }

// saveImage's conversion on the device; leaves the bytes in a device buffer owned by the context.
int pt_ctx_save_u8_device(PtContext* c, float samples, const uint8_t** rgb8_dev) {
  if (need(c, "pt_save_u8")) return -1;
  Ctx& g = *c;
  const int W = g.cam.resolution[0];
  if (!(samples > 0.0f)) return pt_fail("pt_save_u8: samples must be positive");
  if (admit(g, "pt_save_u8", kUniform | kNoExtras)) return -1;
  if (g.pixel_begin % W || g.N % W || (g.stripe && g.stripe != W))  // (its own rule: the rows of a striped frame need not be contiguous)
    return pt_fail("pt_save_u8: the tile must consist of whole image rows (begin %d, count %d, stripe %d, width %d)", g.pixel_begin, g.N, g.stripe, W);
  HIP_OK(hipSetDevice(g.device));
  if (ensure(g, g.d_rgb8, 3 * (size_t)g.N)) return -1;
  g.k->save_u8(g.stream, g.N, W, samples, g.d_image, g.d_rgb8);
  HIP_OK(hipGetLastError());
  if (rgb8_dev) *rgb8_dev = g.d_rgb8;
  return 0;
}
int pt_ctx_save_u8(PtContext* c, float samples, uint8_t* rgb8_host) {
  return copy_out(c, "pt_save_u8", rgb8_host, 3, [&](const uint8_t** d) { return pt_ctx_save_u8_device(c, samples, d); });
}

int pt_ctx_preview_rgba8_device(PtContext* c, int iterations, void* rgba_dev) {
  if (need(c, "pt_preview_rgba8_device")) return -1;
  if (!rgba_dev || iterations <= 0) return pt_fail("pt_preview_rgba8_device: bad argument");
  if (admit(*c, "pt_preview_rgba8_device", kUniform | kNoExtras | kOnDevice)) return -1;
  c->k->preview(c->stream, c->N, iterations, c->d_image, reinterpret_cast<uchar4*>(rgba_dev));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}

int pt_ctx_preview_rgba8(PtContext* c, int iterations, uint8_t* rgba_host) {
  if (need(c, "pt_preview_rgba8")) return -1;
  if (!rgba_host || iterations <= 0) return pt_fail("pt_preview_rgba8: bad argument");
  if (admit(*c, "pt_preview_rgba8", kUniform | kNoExtras | kOnDevice)) return -1;
  uchar4* d = nullptr;
  HIP_OK(hipMalloc((void**)&d, (size_t)c->N * 4));
  c->k->preview(c->stream, c->N, iterations, c->d_image, d);
  hipError_t e = hipMemcpyAsync(rgba_host, d, (size_t)c->N * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return pt_fail("pt_preview_rgba8: %s", hipGetErrorString(e));
  return 0;
}

int pt_ctx_get_stats(PtContext* c, PtStats* out) {
  if (need(c, "pt_get_stats")) return -1;
  if (!out) return pt_fail("pt_get_stats: null");
  if (pt_ctx_sync(c)) return -1;
  Ctx& g = *c;
  std::memset(out, 0, sizeof(*out));
  unsigned long long st[PT_MAX_DEPTH];
  HIP_OK(hipMemcpy(st, g.d_stats, sizeof(st), hipMemcpyDeviceToHost));
  for (int d = 0; d < PT_MAX_DEPTH; ++d) out->live_rays[d] = (int64_t)st[d];
  out->samples = g.samples;
  out->intersect_launches = g.isect_launches;
  out->intersect_ms = g.isect_ms;
  out->render_ms = g.render_ms;
  out->num_cus = g.num_cus;
  out->grid_blocks = g.grid_paths > 0 ? g.grid_paths : g.grid_isect;
  out->num_queues = g.qs.Q;
  out->iters_per_batch = g.K;
  out->device_bytes = g.device_bytes;
  out->primary_fused = g.fuse_primary ? 1 : 0;
  out->bounces_fused = g.fuse_bounces ? 1 : 0;
  out->arith = g.arith;
  if (tables(g).use_grid && g.fuse_bounces) {
    const int* res = g.grids[g.grid_pick].shape.res;
    out->grid_cells = res[0] * res[1] * res[2];
  }
  out->tight_leaves = g.tight_leaves;
  out->record_form = g.record_form;
  out->gather_form = g.gather_form;
  out->inline_gathers = g.inline_gathers;
  out->primary_launches = g.primary_launches;
  out->paths_waves = 0;
  if (g.qs.deal && g.grid_paths > 0) {  // the table the NEXT batch's k_paths launch will read (ptd::Queues::deal)
    const ptk::DealMap dm = ptk::deal_map(g.qs);
    std::vector<int32_t> first((size_t)dm.made_for() + 1);  // first(0 .. Q)
    HIP_OK(hipMemcpy(first.data(), g.qs.deal + dm.first(0), first.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (first[dm.made_for()] == g.qs.paths_W) {
      int lo = first[1] - first[0], hi = lo;
      for (int q = 1; q < g.qs.Q; ++q) lo = std::min(lo, first[q + 1] - first[q]), hi = std::max(hi, first[q + 1] - first[q]);
      out->paths_waves = std::min(lo, 0xffff) << 16 | std::min(hi, 0xffff);
    }
  }
  return 0;
}

int pt_ctx_reset_stats(PtContext* c) {
  if (need(c, "pt_reset_stats")) return -1;
  if (pt_ctx_sync(c)) return -1;
  Ctx& g = *c;
  // on the render stream (created non-blocking: the null stream would not be ordered against it)
  HIP_OK(hipMemsetAsync(g.d_stats, 0, PT_MAX_DEPTH * sizeof(unsigned long long), g.stream));
  HIP_OK(hipStreamSynchronize(g.stream));
  g.samples = 0;
  g.isect_ms = g.render_ms = 0;
  g.isect_launches = 0;
  return 0;
}

int pt_ctx_clear(PtContext* c) {
  if (need(c, "pt_clear")) return -1;
  if (pt_ctx_sync(c)) return -1;
  HIP_OK(hipMemsetAsync(c->d_image, 0, 3 * (size_t)c->N * sizeof(float), c->stream));
  if (c->d_feat) HIP_OK(hipMemsetAsync(c->d_feat, 0, (size_t)PT_FEATURE_PLANES * c->N * sizeof(float4), c->stream));  // sums and object ids
  if (c->d_noise) HIP_OK(hipMemsetAsync(c->d_noise, 0, pt_noise_state_bytes((size_t)c->N), c->stream));
  c->noise_groups = 0;
  c->noise_iters = c->rendered = 0;
  if (c->d_acnt) HIP_OK(hipMemsetAsync(c->d_acnt, 0, (size_t)c->N * sizeof(ptad::Cnt), c->stream));  // back to the uniform state; nothing is freed
  c->adaptive = false;
  c->adaptive_rounds = 0;
  c->adaptive_last = 0;
  c->hist_current = c->feat_fresh = false;
  c->hist_var_current = 0;  // the history's current planes are absent; its kept planes stay (pt_history.h)
  c->fb_current = c->fb_pending = false;  // ... and so are the feedback's FC and P; FK stays
  if (c->d_hist_extra) HIP_OK(hipMemsetAsync(c->d_hist_extra, 0, (size_t)c->N * sizeof(float), c->stream));  // the extras belong to the image
  c->hist_extra = false;
  c->hist_noise = c->hist_ne = false;  // the blend's noise plane W (and NE beside it) described the image that was
  c->probe_checked = c->probe_applied = false;  // the probes' L belongs to C; PK stays
  if (c->conv) {  // forget the curve, re-arm the capture (a supplied frame stays)
    HIP_OK(hipMemsetAsync(c->d_sse, 0xff, (size_t)PT_CONVERGENCE_CAPACITY * sizeof(double), c->stream));
    c->conv_last = 0;
    if (c->conv > 0) c->conv_have_ref = false;
  }
  return pt_ctx_reset_stats(c);
}

// ---- moving the camera -----------------------------------------------------------------------
}  // extern "C"
// What pt_set_camera refuses, under the name `who`; a group asks every context before it changes one.
int pt_ctx_camera_refusal(const PtContext* c, const PtCamera* cam, const char* who) {
  if (need(c, who) || admit(*c, who, kNotFailed)) return -1;
  if (!cam) return pt_fail("%s: null camera", who);
  if (cam->resolution[0] != c->cam.resolution[0] || cam->resolution[1] != c->cam.resolution[1])
    return pt_fail("%s: resolution %dx%d differs from the renderer's %dx%d; a new resolution needs pt_init", who, cam->resolution[0], cam->resolution[1],
                   c->cam.resolution[0], c->cam.resolution[1]);
  const struct {
    const char* name;
    const float* v;
    int n;
  } fields[] = {{"position", cam->position, 3}, {"view", cam->view, 3}, {"up", cam->up, 3}, {"right", cam->right, 3}, {"fov", cam->fov, 2}, {"pixelLength", cam->pixelLength, 2}};
  for (const auto& f : fields)
    for (int i = 0; i < f.n; ++i)
      if (!std::isfinite(f.v[i])) return pt_fail("%s: camera %s[%d] is not finite", who, f.name, i);
  return 0;
}
// ... and what pt_set_camera_ex adds: a flag bit that is not defined, looked at after the null camera
int pt_ctx_camera_refusal_ex(const PtContext* c, const PtCamera* cam, uint32_t flags, const char* who) {
  if (need(c, who) || admit(*c, who, kNotFailed)) return -1;
  if (!cam) return pt_fail("%s: null camera", who);
  if (flags & ~(uint32_t)PT_SET_CAMERA_DEVICE_TABLES) return pt_fail("%s: undefined flag bit(s) 0x%x (defined: PT_SET_CAMERA_DEVICE_TABLES = 0x%x)", who, flags & ~(uint32_t)PT_SET_CAMERA_DEVICE_TABLES, PT_SET_CAMERA_DEVICE_TABLES);
  return pt_ctx_camera_refusal(c, cam, who);
}
// What pt_set_geoms refuses, under the name `who`; a group asks every context before it changes one.
int pt_ctx_geoms_refusal(const PtContext* c, const PtGeom* geoms, int num_geoms, const char* who) {
  if (need(c, who) || admit(*c, who, kNotFailed)) return -1;
  if (!geoms) return pt_fail("%s: null geoms", who);
  const std::vector<PtGeom>& have = c->camera_base.geoms;
  if (num_geoms != (int)have.size())
    return pt_fail("%s: %d geoms, but the renderer was created with %d; adding or removing objects needs pt_init", who, num_geoms, (int)have.size());
  for (int i = 0; i < num_geoms; ++i)
    if (geoms[i].type != have[(size_t)i].type || geoms[i].materialid != have[(size_t)i].materialid)
      return pt_fail("%s: geom %d has type %d and material %d, the renderer's has type %d and material %d; only the transforms may change", who, i, geoms[i].type,
                     geoms[i].materialid, have[(size_t)i].type, have[(size_t)i].materialid);
  for (int i = 0; i < num_geoms; ++i)
    for (const float* m : {geoms[i].transform, geoms[i].inverseTransform, geoms[i].invTranspose})
      for (int k = 0; k < 16; ++k)
        if (!std::isfinite(m[k])) return pt_fail("%s: geom %d has a matrix element that is not finite", who, i);
  return 0;
}
// What pt_set_materials refuses, under the name `who`; a group asks every context before it changes one.
int pt_ctx_materials_refusal(const PtContext* c, const PtMaterial* materials, int num_materials, const char* who) {
  if (need(c, who) || admit(*c, who, kNotFailed)) return -1;
  if (!materials) return pt_fail("%s: null materials", who);
  if (num_materials != (int)c->materials.size())
    return pt_fail("%s: %d materials, but the renderer was created with %d; adding or removing materials needs pt_init", who, num_materials, (int)c->materials.size());
  for (int i = 0; i < num_materials; ++i) {
    const PtMaterial& m = materials[i];
    const struct {
      const char* name;
      const float* v;
      int n;
    } fields[] = {{"color", m.color, 3}, {"specular_color", m.specular_color, 3}, {"hasReflective", &m.hasReflective, 1}, {"hasRefractive", &m.hasRefractive, 1}, {"emittance", &m.emittance, 1}};
    for (const auto& f : fields)
      for (int k = 0; k < f.n; ++k)
        if (!std::isfinite(f.v[k])) return pt_fail("%s: %s of material %d is not finite", who, f.name, i);
  }
  return 0;
}
namespace {
template <typename T>
void release(Ctx& g, const T* dev, size_t count) {  // a table of `count` entries that dalloc() gave: back to the device
  if (!dev) return;
  void* p = const_cast<T*>(dev);
  (void)hipFree(p);
  g.allocs.erase(std::remove(g.allocs.begin(), g.allocs.end(), p), g.allocs.end());
  g.device_bytes -= (int64_t)std::max<size_t>(count * sizeof(T), 16);
}
template <typename T>
int reupload(const T* dev, const std::vector<T>& v) {  // into a table of unchanged size
  HIP_OK(hipMemcpy(const_cast<T*>(dev), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}
// The grid: the one choose_traversal() kept is rebuilt at its resolution (gr), or dropped (nullptr: the probe preferred the BVH scan,
// or build_grid refuses for this camera or these geoms).  Cell table and records are reused where their sizes are unchanged.
int move_grid(Ctx& g, const pt::Grid* gr) {
  if (!g.grids.empty()) {
    Ctx::DeviceGrid& d = g.grids[g.grid_pick];
    if (gr && gr->start.size() == d.start.size() && gr->items.size() == d.items && gr->items_b.empty() == (d.d_items_b == d.d_items)) {
      if (reupload(d.d_start, gr->start) || reupload(d.d_items, gr->items)) return -1;
      if (!gr->items_b.empty() && reupload(d.d_items_b, gr->items_b)) return -1;
      d.shape = gr->shape, d.guard = gr->guard, d.start = gr->start, d.start_stale = false;
      return 0;
    }
    free_grid(g, d);
    g.grids.clear();
    g.grid_pick = 0;
  }
  return gr ? upload_grid(g, *gr) : 0;
}
// The camera-dependent tables for g.cam, on the device (setup()'s build_scene_tables + upload_tables for that part).  The stream is idle.
int move_tables(Ctx& g) {
  pt::HostTables t;
  std::memcpy(t.root_min, g.scene.root_min, 12);
  std::memcpy(t.root_max, g.scene.root_max, 12);
  const bool center_half = g.k->boxes_center_half != 0;
  pt::camera_tables(t, g.camera_base, g.cam.position, g.debug_flags, center_half, g.grid_request);
  ptk::SceneTables& s = g.scene;
  if (reupload(s.nodes, t.nodes) || reupload(s.top, t.top)) return -1;
  if (center_half && (reupload(s.nodes_b, t.nodes_b) || reupload(s.top_b, t.top_b))) return -1;
  s.cull_margin = t.cull_margin;
  g.tight_leaves = t.tight_leaves;
  return move_grid(g, t.grids.empty() ? nullptr : &t.grids[0]);
}


// The first device-path move of a renderer: camera_base on the device (base nodes, base top list, the fields of PtGeom the build reads)
// and the build's workspace, sized for the grid the renderer rebuilds (grid_request never changes after setup()).
int ensure_device_base(Ctx& g) {
  Ctx::DeviceBase& b = g.device_base;
  if (b.ready) return 0;
  const pt::CameraBase& cb = g.camera_base;
  std::vector<ptct::DeviceGeom> geoms(cb.geoms.size());
  for (size_t i = 0; i < geoms.size(); ++i) {
    geoms[i] = ptct::DeviceGeom{};
    std::memcpy(geoms[i].inv, cb.geoms[i].inverseTransform, sizeof(geoms[i].inv));
    geoms[i].type = cb.geoms[i].type;
  }
  if (!(b.nodes = upload(g, cb.nodes)) || !(b.top = upload(g, cb.top)) || !(b.geoms = upload(g, geoms))) return -1;
  if (b.rec) return b.ready = true, 0;  // after pt_ctx_set_geoms: the workspace follows the grid's resolution and the leaf count, which stay
  if (dalloc(g, &b.rec, 1)) return -1;
  if (g.grid_request.kind == pt::GridRequest::kFixed) {
    int64_t ncell = 1, leaves = 0;
    for (int a = 0; a < 3; ++a) ncell *= std::min(512, std::max(1, g.grid_request.res[a]));
    for (const ptd::Node& n : cb.nodes) leaves += n.geom >= 0 ? 1 : 0;
    if (ncell <= ptct::kDeviceMaxCells) {  // (else every device-path move falls back to the host: no workspace)
      // a grid that is not forced is refused beyond 64 references per leaf (build_grid), any grid beyond kMaxRefs
      b.scratch_cap = (size_t)((g.debug_flags & 256) ? ptct::kMaxRefs : std::min<int64_t>(ptct::kMaxRefs, 64 * leaves));
      if (dalloc(g, &b.count, (size_t)ncell) || dalloc(g, &b.sums, pt_camera_tables_scan_blocks((size_t)ncell)) || dalloc(g, &b.scratch, b.scratch_cap)) return -1;
    }
  }
  b.ready = true;
  return 0;
}

// move_tables() with the build on the device (csrc/pt_camera_tables.hip): the host computes the scalars as camera_tables() and build_grid()
// do, the kernels everything per node, per top entry and per (leaf, cell) reference.  *fallback != 0: a limit of the device build
// (PT_DEVICE_TABLES_*) was met and nothing the renderer reads was left half built that move_tables() does not write again.
int move_tables_device(Ctx& g, int32_t* fallback) {
  *fallback = 0;
  const pt::CameraBase& cb = g.camera_base;
  const bool center_half = g.k->boxes_center_half != 0;
  const bool forced = (g.debug_flags & 256) != 0;
  ptk::SceneTables& s = g.scene;
  ptct::BuildArgs a{};
  a.num_nodes = (int32_t)cb.nodes.size(), a.num_top = (int32_t)cb.top.size();
  a.tighten = ((int)cb.nodes.size() >= pt::kTightNodes && !(g.debug_flags & 2048)) ? 1 : 0;
  a.center_half = center_half ? 1 : 0;
  pt::origin_region(s.root_min, s.root_max, g.cam.position, a.origin_lo, a.origin_hi);
  a.magnitude = pt::scene_magnitude(s.root_min, s.root_max, g.cam.position);
  // the grid's scalars, as camera_tables() and build_grid() compute them for a kFixed request
  pt::GridShape shape{};
  bool want_grid = g.grid_request.kind == pt::GridRequest::kFixed && !(g.debug_flags & 512);
  if (want_grid) {
    double cam_mag = 0.0;
    for (int k = 0; k < 3; ++k) cam_mag = std::max(cam_mag, std::fabs((double)g.cam.position[k]));
    int64_t ncell = 0;
    size_t guard = 0;
    const pt::GridVerdict v = pt::device_grid_scalars(s.root_min, s.root_max, cam_mag, g.grid_request.res, (int64_t)cb.geoms.size(), a.frame, shape, &ncell, &guard);
    if (v == pt::kGridCells) return *fallback = PT_DEVICE_TABLES_CELLS, 0;
    want_grid = v == pt::kGridBuild;
    a.ncell = (uint32_t)ncell, a.guard = (uint32_t)guard;
  }
  if (ensure_device_base(g)) return -1;
  const Ctx::DeviceBase& b = g.device_base;
  ptd::Node* nodes_b = center_half ? const_cast<ptd::Node*>(s.nodes_b) : nullptr;
  ptd::TopEntry* top_b = center_half ? const_cast<ptd::TopEntry*>(s.top_b) : nullptr;
  if (pt_camera_tables_nodes_launch(g.stream, a, b.nodes, b.top, b.geoms, const_cast<ptd::Node*>(s.nodes), nodes_b, const_cast<ptd::TopEntry*>(s.top), top_b, b.rec))
    return -1;
  if (want_grid && pt_camera_tables_count_launch(g.stream, a, s.nodes, b.count, b.rec)) return -1;
  ptct::BuildRecord rec{};  // the one readback: references, longest list, tightened leaves
  HIP_OK(hipMemcpyAsync(&rec, b.rec, sizeof(rec), hipMemcpyDeviceToHost, g.stream));
  HIP_OK(hipStreamSynchronize(g.stream));
  {
    const float extent = std::max(1.0f, (float)pt::scene_magnitude(s.root_min, s.root_max, g.cam.position));
    s.cull_margin = 1e-3f * cb.max_xf + 1e-4f * extent;
  }
  g.tight_leaves = (int)rec.tight;
  if (want_grid) {  // build_grid's refusals on what the kernels counted
    const pt::GridVerdict v = pt::device_grid_counted(forced, ((int64_t)cb.nodes.size() + 1) / 2, rec.refs, rec.longest, b.scratch_cap);
    if (v == pt::kGridList) return *fallback = PT_DEVICE_TABLES_LIST, 0;
    want_grid = v == pt::kGridBuild;
  }
  // the grid's buffers: reused where the sizes are unchanged, else replaced (move_tables' rule)
  if (!g.grids.empty()) {
    Ctx::DeviceGrid& d = g.grids[g.grid_pick];
    const bool keep = want_grid && (size_t)a.ncell + 1 + 2 * (size_t)a.guard == d.start.size() && (size_t)rec.refs == d.items && center_half == (d.d_items_b != d.d_items);
    if (!keep) {
      free_grid(g, d);
      g.grids.clear();
      g.grid_pick = 0;
    }
  }
  if (want_grid) {
    if (g.grids.empty()) {
      Ctx::DeviceGrid d{shape, a.guard, nullptr, nullptr, nullptr, 0, {}};
      const int64_t before = g.device_bytes;
      uint32_t* start = nullptr;
      ptd::Node *items = nullptr, *items_b = nullptr;
      if (dalloc(g, &start, (size_t)a.ncell + 1 + 2 * (size_t)a.guard) || dalloc(g, &items, (size_t)rec.refs)) return -1;
      if (center_half && dalloc(g, &items_b, (size_t)rec.refs)) return -1;
      d.d_start = start, d.d_items = items, d.d_items_b = center_half ? items_b : items;
      d.bytes = (size_t)(g.device_bytes - before);
      d.items = (size_t)rec.refs;
      d.start.assign((size_t)a.ncell + 1 + 2 * (size_t)a.guard, 0u);
      g.grids.push_back(d);
    }
    Ctx::DeviceGrid& d = g.grids[g.grid_pick];
    d.shape = shape, d.guard = a.guard, d.start_stale = true;
    if (pt_camera_tables_grid_launch(g.stream, a, s.nodes, b.geoms, b.count, b.sums, b.scratch, (uint32_t)rec.refs, const_cast<uint32_t*>(d.d_start),
                                     const_cast<ptd::Node*>(d.d_items), center_half ? const_cast<ptd::Node*>(d.d_items_b) : nullptr))
      return -1;
  }
  HIP_OK(hipStreamSynchronize(g.stream));  // (so that PtSetCameraTimes.tables_ms holds the build, not its launches)
  return 0;
}

int set_camera(PtContext* c, const PtCamera* cam, uint32_t flags) {  // after the refusals
  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
  const auto t0 = clock::now();
  Ctx& g = *c;
  if (pt_ctx_sync(c)) return -1;
  take_camera(g, *cam);
  PtSetCameraTimes times{};
  if (flags & PT_SET_CAMERA_DEVICE_TABLES) {
    times.path = 1;
    if (move_tables_device(g, &times.fallback)) return g.failed = true, -1;
  }
  if (!(flags & PT_SET_CAMERA_DEVICE_TABLES) || times.fallback) {
    times.path = 0;
    if (move_tables(g)) return g.failed = true, -1;  // (tables half replaced: nothing may render from them)
  }
  times.tables_ms = ms_since(t0);
  const auto t1 = clock::now();
  plan_launch(g);
  g.record_form = g.gather_form = 0;
  if (Ctx* w = g.worker) {  // the worker's view of the scene is a copy: camera, table pointers, grid and launch widths again
    static_cast<PtShared&>(*w) = g;
    set_worker_live(*w, w->capacity);
    plan_launch(*w);
    if (rearm_batch_buffers(*w)) return g.failed = true, -1;
  }
  if (rearm_batch_buffers(g)) return g.failed = true, -1;
  if (pt_ctx_clear(c)) return -1;
  times.rearm_ms = ms_since(t1);
  times.total_ms = ms_since(t0);
  g.camera_times = times;
  g.setup_times.set_camera_ms = times.total_ms;
  g.setup_times.set_camera_calls += 1;
  return 0;
}

// A table of the renderer with new contents: into the buffer it has where the length is unchanged, else into a new one.
template <typename T>
int replace_table(Ctx& g, const T*& dev, size_t old_count, const std::vector<T>& v) {
  if (v.size() == old_count) return reupload(dev, v);
  release(g, dev, old_count);
  return (dev = upload(g, v)) ? 0 : -1;
}
int set_geoms(PtContext* c, const PtGeom* geoms, int num_geoms) {  // after the refusals
  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
  const auto t0 = clock::now();
  Ctx& g = *c;
  if (pt_ctx_sync(c)) return -1;
  PtSetGeomsTimes times{};
  // pt_init's build for these geoms and the renderer's camera, at the grid resolution pt_init chose; no materials: their table stays
  const bool center_half = g.k->boxes_center_half != 0;
  PtSceneDesc desc{};
  desc.geoms = geoms, desc.num_geoms = num_geoms;
  desc.camera = g.cam;
  pt::CameraBase base;
  const pt::HostTables t = pt::build_scene_tables(desc, g.debug_flags, center_half, g.grid_request, &base);
  times.build_ms = ms_since(t0);
  const auto t1 = clock::now();
  ptk::SceneTables& s = g.scene;
  const size_t old_nodes = (size_t)s.num_nodes, old_top = (size_t)s.num_top;
  g.failed = true;  // (tables half replaced: nothing may render from them) until everything below has succeeded
  if (replace_table(g, s.nodes, old_nodes, t.nodes) || replace_table(g, s.top, old_top, t.top) || replace_table(g, s.geoms, (size_t)s.num_geoms, t.geoms)) return -1;
  if (center_half) {
    if (replace_table(g, s.nodes_b, old_nodes, t.nodes_b) || replace_table(g, s.top_b, old_top, t.top_b)) return -1;
  } else {
    s.nodes_b = s.nodes, s.top_b = s.top;
  }
  s.num_nodes = (int)t.nodes.size(), s.num_top = (int)t.top.size();
  std::memcpy(s.root_min, t.root_min, 12);
  std::memcpy(s.root_max, t.root_max, 12);
  s.cull_margin = t.cull_margin;
  s.top_xor = t.top_xor;
  g.tight_leaves = t.tight_leaves;
  if (move_grid(g, t.grids.empty() ? nullptr : &t.grids[0])) return -1;
  // the device copy of the camera-independent tables belongs to the old geoms: the next device-path move uploads the new one
  if (Ctx::DeviceBase& b = g.device_base; b.ready) {
    release(g, b.nodes, g.camera_base.nodes.size()), release(g, b.top, g.camera_base.top.size()), release(g, b.geoms, g.camera_base.geoms.size());
    b.nodes = nullptr, b.top = nullptr, b.geoms = nullptr, b.ready = false;
  }
  g.camera_base = std::move(base);
  g.hist_motion.geoms_stale = true, g.hist_motion.fresh = false;  // (the next capture keeps these geoms; K and the kept geoms stay until then)
  g.probe_geoms_stale = g.probe_geoms_changed = true;  // (the next keep copies these geoms; the next check compares them with the kept ones)
  times.upload_ms = ms_since(t1);
  const auto t2 = clock::now();
  plan_launch(g);
  g.record_form = g.gather_form = 0;
  if (Ctx* w = g.worker) {  // as in set_camera()
    static_cast<PtShared&>(*w) = g;
    set_worker_live(*w, w->capacity);
    plan_launch(*w);
    if (rearm_batch_buffers(*w)) return -1;
  }
  if (rearm_batch_buffers(g)) return -1;
  g.failed = false;
  if (pt_ctx_clear(c)) return -1;
  times.rearm_ms = ms_since(t2);
  times.total_ms = ms_since(t0);
  g.geoms_times = times;
  return 0;
}
int set_materials(PtContext* c, const PtMaterial* materials, int num_materials) {  // after the refusals
  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
  const auto t0 = clock::now();
  Ctx& g = *c;
  if (pt_ctx_sync(c)) return -1;
  PtSetMaterialsTimes times{};
  // pt_init's table for these materials, into the buffer the renderer has: the count is the renderer's, so nothing is allocated
  if (reupload(g.scene.mats, pt::material_table(materials, num_materials))) return g.failed = true, -1;
  g.materials.assign(materials, materials + num_materials);
  g.hist_reject_stale = g.hist_emitter_stale = true;  // the per-geom tables of the history follow the materials: rebuilt at their next use
  g.hist_materials.stale = true, g.hist_materials.fresh = false;  // (the next capture keeps these materials; K and the kept materials stay until then)
  g.probe_materials_stale = g.probe_materials_changed = true;     // (the next keep copies these materials; the next check compares them with the kept ones)
  times.upload_ms = ms_since(t0);
  const auto t1 = clock::now();
  // Whether a camera ray survives depth 0 follows the emittance of what it hits, and the primary kernel's records are reused from
  // batch to batch: the whole re-arm of a camera move
  plan_launch(g);
  g.record_form = g.gather_form = 0;
  if (Ctx* w = g.worker) {  // as in set_camera()
    static_cast<PtShared&>(*w) = g;
    set_worker_live(*w, w->capacity);
    plan_launch(*w);
    if (rearm_batch_buffers(*w)) return g.failed = true, -1;
  }
  if (rearm_batch_buffers(g)) return g.failed = true, -1;
  if (pt_ctx_clear(c)) return -1;
  times.rearm_ms = ms_since(t1);
  times.total_ms = ms_since(t0);
  g.materials_times = times;
  return 0;
}
}  // namespace

namespace ptc {
int grid_start_host(Ctx& g, Ctx::DeviceGrid& d) {
  if (!d.start_stale) return 0;
  HIP_OK(hipSetDevice(g.device));
  HIP_OK(hipStreamSynchronize(g.stream));
  HIP_OK(hipMemcpy(d.start.data(), d.d_start, d.start.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  d.start_stale = false;
  return 0;
}
}  // namespace ptc
extern "C" {

int pt_ctx_set_camera(PtContext* c, const PtCamera* cam) {
  if (pt_ctx_camera_refusal(c, cam, "pt_set_camera")) return -1;
  return set_camera(c, cam, 0u);
}
int pt_ctx_set_camera_ex(PtContext* c, const PtCamera* cam, uint32_t flags) {
  if (pt_ctx_camera_refusal_ex(c, cam, flags, "pt_set_camera_ex")) return -1;
  return set_camera(c, cam, flags);
}
int pt_ctx_set_geoms(PtContext* c, const PtGeom* geoms, int num_geoms) {
  if (pt_ctx_geoms_refusal(c, geoms, num_geoms, "pt_set_geoms")) return -1;
  return set_geoms(c, geoms, num_geoms);
}
int pt_ctx_get_set_geoms_times(PtContext* c, PtSetGeomsTimes* out) {
  if (need(c, "pt_get_set_geoms_times")) return -1;
  if (!out) return pt_fail("pt_get_set_geoms_times: null");
  *out = c->geoms_times;
  return 0;
}
int pt_ctx_set_materials(PtContext* c, const PtMaterial* materials, int num_materials) {
  if (pt_ctx_materials_refusal(c, materials, num_materials, "pt_set_materials")) return -1;
  return set_materials(c, materials, num_materials);
}
int pt_ctx_get_set_materials_times(PtContext* c, PtSetMaterialsTimes* out) {
  if (need(c, "pt_get_set_materials_times")) return -1;
  if (!out) return pt_fail("pt_get_set_materials_times: null");
  *out = c->materials_times;
  return 0;
}
int pt_ctx_get_set_camera_times(PtContext* c, PtSetCameraTimes* out) {
  if (need(c, "pt_get_set_camera_times")) return -1;
  if (!out) return pt_fail("pt_get_set_camera_times: null");
  *out = c->camera_times;
  return 0;
}

int pt_ctx_get_setup_times(PtContext* c, PtSetupTimes* out) {
  if (need(c, "pt_get_setup_times")) return -1;
  if (!out) return pt_fail("pt_get_setup_times: null");
  *out = c->setup_times;
  return 0;
}

int pt_camera_tables_host(const PtSceneDesc* scene, const PtCamera* cam, int debug_flags, int center_half, int32_t grid_res_out[3],
                          int32_t* tight_leaves, int32_t* differing) {
  if (!scene || !cam || !grid_res_out || !tight_leaves || !differing || !scene->geoms || scene->num_geoms <= 0 || !scene->materials || scene->num_materials <= 0)
    return pt_fail("pt_camera_tables_host: null argument");
  return pt::camera_tables_check(*scene, *cam, debug_flags, center_half != 0, grid_res_out, tight_leaves, differing);
}

int pt_camera_grid_host(const PtTableNode* nodes, int num_nodes, const int32_t* geom_types, int num_geoms, const float root_min[3],
                        const float root_max[3], double coord_mag, const int32_t res[3], int center_half, PtCameraGridResult* out,
                        uint32_t* start, uint64_t start_cap, PtGridRecord* items, PtGridRecord* items_b, uint64_t items_cap) {
  if (const char* why = pt::camera_grid_refusal(nodes, num_nodes, geom_types, num_geoms, root_min, root_max, coord_mag, res, out))
    return pt_fail("pt_camera_grid_host: %s", why);
  const bool query = !start && !items;
  if (!query && (!start || !items || (center_half && !items_b))) return pt_fail("pt_camera_grid_host: null argument");
  pt::Grid grid;
  pt::camera_grid_host(reinterpret_cast<const ptd::Node*>(nodes), num_nodes, geom_types, num_geoms, root_min, root_max, coord_mag, res, center_half != 0, out, grid);
  if (out->status != 0 || query) return 0;
  if (grid.start.size() > start_cap || grid.items.size() > items_cap)
    return pt_fail("pt_camera_grid_host: the grid needs %zu words and %zu records, the arrays hold %llu and %llu", grid.start.size(), grid.items.size(),
                   (unsigned long long)start_cap, (unsigned long long)items_cap);
  std::memcpy(start, grid.start.data(), grid.start.size() * sizeof(uint32_t));
  if (!grid.items.empty()) std::memcpy(items, grid.items.data(), grid.items.size() * sizeof(ptd::Node));
  if (center_half && !grid.items_b.empty()) std::memcpy(items_b, grid.items_b.data(), grid.items_b.size() * sizeof(ptd::Node));
  return 0;
}

// ---- convergence metric ---------------------------------------------------------------------
int pt_ctx_set_reference(PtContext* c, const float* rgb_avg_host) {
  if (need(c, "pt_set_reference")) return -1;
  if (!rgb_avg_host) return pt_fail("pt_set_reference: null image");
  if (c->conv != -1) return pt_fail("pt_set_reference: the renderer was created with PtOptions.convergence = %d, not -1", c->conv);
  if (pt_ctx_sync(c)) return -1;
  HIP_OK(hipMemcpyAsync(c->d_ref, rgb_avg_host, 3 * (size_t)c->N * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  c->conv_have_ref = true;
  return 0;
}

int pt_ctx_get_convergence(PtContext* c, int iter_first, int iter_count, double* sse) {
  if (need(c, "pt_get_convergence")) return -1;
  if (!c->conv) return pt_fail("pt_get_convergence: the renderer was created with PtOptions.convergence = 0 (metric off)");
  if (iter_count < 0 || (iter_count > 0 && !sse)) return pt_fail("pt_get_convergence: bad argument");
  if (pt_ctx_sync(c)) return -1;
  for (int j = 0; j < iter_count; ++j) sse[j] = -1.0;
  const int64_t lo = std::max<int64_t>(iter_first, 1), hi = std::min<int64_t>((int64_t)iter_first + iter_count, (int64_t)PT_CONVERGENCE_CAPACITY + 1);
  if (lo >= hi) return 0;
  double* dst = sse + (lo - iter_first);
  HIP_OK(hipMemcpy(dst, c->d_sse + (lo - 1), (size_t)(hi - lo) * sizeof(double), hipMemcpyDeviceToHost));
  for (int64_t j = 0; j < hi - lo; ++j)
    if (!(dst[j] >= 0.0)) dst[j] = -1.0;  // the "no value" pattern is a NaN
  return 0;
}

int pt_ctx_iterations_to_clean(PtContext* c, float threshold_db, int* iteration) {
  if (need(c, "pt_iterations_to_clean")) return -1;
  if (!iteration) return pt_fail("pt_iterations_to_clean: null output");
  std::vector<double> sse((size_t)std::max(c->conv_last, 0));
  if (pt_ctx_get_convergence(c, 1, (int)sse.size(), sse.data())) return -1;
  *iteration = -1;
  for (size_t i = 0; i < sse.size(); ++i)
    if (sse[i] >= 0.0 && pt_psnr_from_sse(sse[i], c->N) > threshold_db) {
      *iteration = (int)i + 1;
      break;
    }
  return 0;
}

// ---- the reference's single-instance API (pathtrace.h) on a default context -------------
int pt_free(void) {  // pathtraceFree() before init / twice is legal (main.cpp:134)
  PtContext* c = g_default;
  g_default = nullptr;
  destroy(c);
  return 0;
}
int pt_init(const PtSceneDesc* sc, const PtOptions* opt) {
  pt_free();
  return pt_ctx_create(sc, opt, &g_default);
}
int pt_render(int iter_first, int iter_count) { return pt_ctx_render(g_default, iter_first, iter_count); }
int pt_sync(void) { return pt_ctx_sync(g_default); }
int pt_readback(float* out) { return pt_ctx_readback(g_default, out); }
int pt_readback_device(void* out) { return pt_ctx_readback_device(g_default, out); }
int pt_save_u8(float samples, uint8_t* rgb8_host) { return pt_ctx_save_u8(g_default, samples, rgb8_host); }
int pt_preview_rgba8(int iterations, uint8_t* rgba_host) { return pt_ctx_preview_rgba8(g_default, iterations, rgba_host); }
int pt_preview_rgba8_device(int iterations, void* rgba_dev) { return pt_ctx_preview_rgba8_device(g_default, iterations, rgba_dev); }
int pt_get_stats(PtStats* out) { return pt_ctx_get_stats(g_default, out); }
int pt_reset_stats(void) { return pt_ctx_reset_stats(g_default); }
int pt_clear(void) { return pt_ctx_clear(g_default); }
int pt_set_camera(const PtCamera* cam) { return pt_ctx_set_camera(g_default, cam); }
int pt_set_camera_ex(const PtCamera* cam, uint32_t flags) { return pt_ctx_set_camera_ex(g_default, cam, flags); }
int pt_get_set_camera_times(PtSetCameraTimes* out) { return pt_ctx_get_set_camera_times(g_default, out); }
int pt_set_geoms(const PtGeom* geoms, int num_geoms) { return pt_ctx_set_geoms(g_default, geoms, num_geoms); }
int pt_get_set_geoms_times(PtSetGeomsTimes* out) { return pt_ctx_get_set_geoms_times(g_default, out); }
int pt_set_materials(const PtMaterial* materials, int num_materials) { return pt_ctx_set_materials(g_default, materials, num_materials); }
int pt_get_set_materials_times(PtSetMaterialsTimes* out) { return pt_ctx_get_set_materials_times(g_default, out); }
int pt_get_setup_times(PtSetupTimes* out) { return pt_ctx_get_setup_times(g_default, out); }
int pt_render_features(int iter_first, int iter_count) { return pt_ctx_render_features(g_default, iter_first, iter_count); }
int pt_readback_features(float* planes_host) { return pt_ctx_readback_features(g_default, planes_host); }
int pt_denoise(float samples, const PtDenoiseOptions* opt, float* rgb_avg_host) { return pt_ctx_denoise(g_default, samples, opt, rgb_avg_host); }
int pt_denoise_guided(const PtDenoiseOptions* opt, float* rgb_avg_host) { return pt_ctx_denoise_guided(g_default, opt, rgb_avg_host); }
int pt_denoise_adaptive(const PtDenoiseOptions* opt, float* rgb_avg_host) { return pt_ctx_denoise_adaptive(g_default, opt, rgb_avg_host); }
int pt_noise_fold(void) { return pt_ctx_noise_fold(g_default); }
int pt_get_noise(double* sse, int* groups, int* iterations) { return pt_ctx_get_noise(g_default, sse, groups, iterations); }
int pt_readback_noise(float* planes_host) { return pt_ctx_readback_noise(g_default, planes_host); }
int pt_render_until(int iter_first, int max_iters, int group_iters, float target_db, int* iters_done, float* psnr_db) {
  return pt_ctx_render_until(g_default, iter_first, max_iters, group_iters, target_db, iters_done, psnr_db);
}
int pt_adaptive_round(int iter_first, int group_iters, float fraction) { return pt_ctx_adaptive_round(g_default, iter_first, group_iters, fraction); }
int pt_render_adaptive(int iter_first, int max_iters, int group_iters, float fraction, float target_db, int* iters_done, int64_t* samples_done,
                       float* psnr_db) {
  return pt_ctx_render_adaptive(g_default, iter_first, max_iters, group_iters, fraction, target_db, iters_done, samples_done, psnr_db);
}
int pt_readback_adaptive(int32_t* counts) { return pt_ctx_readback_adaptive(g_default, counts); }
int pt_adaptive_round_threshold(int iter_first, int group_iters, float threshold, float max_fraction, int* above, int* selected) {
  return pt_ctx_adaptive_round_threshold(g_default, iter_first, group_iters, threshold, max_fraction, above, selected);
}
int pt_render_threshold(int iter_first, int max_iters, int group_iters, float threshold, float max_fraction, int min_pixels, int* iters_done,
                        int64_t* samples_done, int* above_left) {
  return pt_ctx_render_threshold(g_default, iter_first, max_iters, group_iters, threshold, max_fraction, min_pixels, iters_done, samples_done, above_left);
}
int pt_adaptive_round_list(int iter_first, int group_iters, const int32_t* list_host, int m, int capacity) {
  return pt_ctx_adaptive_round_list(g_default, iter_first, group_iters, list_host, m, capacity);
}
int pt_resolve(float* rgb_avg_host) { return pt_ctx_resolve(g_default, rgb_avg_host); }
int pt_history_capture(float samples) { return pt_ctx_history_capture(g_default, samples); }
int pt_history_reproject(const PtHistoryOptions* opt) { return pt_ctx_history_reproject(g_default, opt); }
int pt_history_resolve(float samples, float* rgb_avg_host) { return pt_ctx_history_resolve(g_default, samples, rgb_avg_host); }
int pt_readback_history(float* kept_planes, float* current_plane) { return pt_ctx_readback_history(g_default, kept_planes, current_plane); }
int pt_history_drop(void) { return pt_ctx_history_drop(g_default); }
int pt_history_capture_ex(float samples, uint32_t flags) { return pt_ctx_history_capture_ex(g_default, samples, flags); }
int pt_history_reproject_ex(const PtHistoryOptions* opt, uint32_t flags) { return pt_ctx_history_reproject_ex(g_default, opt, flags); }
int pt_history_denoise(float samples, const PtDenoiseOptions* opt, float* rgb_avg_host) { return pt_ctx_history_denoise(g_default, samples, opt, rgb_avg_host); }
int pt_history_denoise_ex(float samples, const PtDenoiseOptions* opt, uint32_t flags, float* rgb_avg_host) {
  return pt_ctx_history_denoise_ex(g_default, samples, opt, flags, rgb_avg_host);
}
int pt_history_denoise_feedback(float samples, const PtDenoiseOptions* opt, const PtHistoryFeedbackOptions* fb, float* rgb_avg_host) {
  return pt_ctx_history_denoise_feedback(g_default, samples, opt, fb, rgb_avg_host);
}
int pt_readback_history_feedback(float* kept, float* current, float* pending) { return pt_ctx_readback_history_feedback(g_default, kept, current, pending); }
int pt_readback_history_variance(float* kept_var, float* current_var) { return pt_ctx_readback_history_variance(g_default, kept_var, current_var); }
int pt_history_round(int iter_first, int group_iters, const PtHistoryRoundOptions* opt, int* fresh, int* selected) {
  return pt_ctx_history_round(g_default, iter_first, group_iters, opt, fresh, selected);
}
int pt_history_round_list(int iter_first, int group_iters, const int32_t* list_host, int m, int capacity) {
  return pt_ctx_history_round_list(g_default, iter_first, group_iters, list_host, m, capacity);
}
int pt_readback_history_extra(float* extra_host) { return pt_ctx_readback_history_extra(g_default, extra_host); }
int pt_history_probe_keep(int iter_first, int iter_count, int phase) { return pt_ctx_history_probe_keep(g_default, iter_first, iter_count, phase); }
int pt_history_probe_check(const PtHistoryProbeOptions* opt, int* probes, int* changed, int* skipped) {
  return pt_ctx_history_probe_check(g_default, opt, probes, changed, skipped);
}
int pt_readback_history_probe(float* kept, float* lam, int* count) { return pt_ctx_readback_history_probe(g_default, kept, lam, count); }
int pt_history_noise(float samples, uint32_t flags, double* sse) { return pt_ctx_history_noise(g_default, samples, flags, sse); }
int pt_readback_history_noise(float* w_host) { return pt_ctx_readback_history_noise(g_default, w_host); }
int pt_history_render_until(int iter_first, int max_iters, int group_iters, float target_db, int* iters_done, float* psnr_db, float* view_psnr_db) {
  return pt_ctx_history_render_until(g_default, iter_first, max_iters, group_iters, target_db, iters_done, psnr_db, view_psnr_db);
}
int pt_history_noise_adaptive(double* sse) { return pt_ctx_history_noise_adaptive(g_default, sse); }
int pt_readback_history_noise_samples(float* ne_host) { return pt_ctx_readback_history_noise_samples(g_default, ne_host); }
int pt_history_round_threshold(int iter_first, int group_iters, float threshold, float max_fraction, int* above, int* selected) {
  return pt_ctx_history_round_threshold(g_default, iter_first, group_iters, threshold, max_fraction, above, selected);
}
int pt_history_render_threshold(int iter_first, int max_iters, int group_iters, float threshold, float max_fraction, int min_pixels, int* iters_done,
                                int64_t* samples_done, int* above_left) {
  return pt_ctx_history_render_threshold(g_default, iter_first, max_iters, group_iters, threshold, max_fraction, min_pixels, iters_done, samples_done, above_left);
}
int pt_history_resolve_adaptive(float* rgb_avg_host) { return pt_ctx_history_resolve_adaptive(g_default, rgb_avg_host); }
int pt_history_capture_adaptive(void) { return pt_ctx_history_capture_adaptive(g_default); }
int pt_history_denoise_adaptive(const PtDenoiseOptions* opt, float* rgb_avg_host) { return pt_ctx_history_denoise_adaptive(g_default, opt, rgb_avg_host); }
int pt_set_reference(const float* rgb_avg_host) { return pt_ctx_set_reference(g_default, rgb_avg_host); }
int pt_get_convergence(int iter_first, int iter_count, double* sse) { return pt_ctx_get_convergence(g_default, iter_first, iter_count, sse); }
int pt_iterations_to_clean(float threshold_db, int* iteration) { return pt_ctx_iterations_to_clean(g_default, threshold_db, iteration); }

}  // extern "C"
