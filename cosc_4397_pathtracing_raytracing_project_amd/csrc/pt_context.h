// pt_context.h — the renderer context and the helpers shared by the translation units that work on it: pt_api.cpp (lifecycle,
// run_batch, readback), pt_post.cpp (what reads or extends a rendered image) and pt_stage.cpp (the stage entry points of the tests).
// Not part of the ABI; nothing outside csrc/ includes it.  The helpers live in namespace ptc, so the library exports them under
// mangled names only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/pt_amd.h"
#include "pt_camera_tables.h"
#include "pt_device.h"
#include "pt_internal.h"
#include "pt_kernels.h"
#include "pt_tables.h"

#define HIP_OK(expr)                                                                                      \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess) return pt_fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

struct EventPair {
  hipEvent_t a, b;
};

// What a worker context (pt_post.cpp ensure_worker) takes from its parent in one assignment: the device and its stream, the kernels,
// the scene as uploaded, every option that decides how a batch is traced.  A member a batch depends on and that does not follow from
// the tile belongs here, so that a worker cannot miss it.  Ownership stays: PtContext::borrowed keeps a worker from freeing the stream,
// and the device memory behind `scene` and `grids` is in the parent's `allocs`.
struct PtShared {
  int device = 0;
  hipStream_t stream = nullptr;
  const ptk::KernelApi* k = nullptr;  // kernels of the selected arithmetic mode
  int arith = 0;
  int num_cus = 0;
  // scene
  PtCamera cam{};
  ptd::Camera dcam{};
  int depth = 0;
  ptk::SceneTables scene{};  // what upload_tables() put on the device; tables() adds the fields that options and launches decide
  int lds_table_bytes = -1;        // SceneTables::lds_table_bytes
  int lds_table_forced = -1;       // PtOptions.lds_table_kb in bytes; -1: KernelApi::lds_table_limit decides
  int primary_pieces = 0;          // BatchInfo::primary_pieces forced by PtOptions.primary_pieces; 0: run_batch decides
  int primary_share = 0;           // BatchInfo::primary_share forced through PT_PRIMARY_PIECES; 0: automatic (primary_share_of)
  int paths_pieces = 0;            // BatchInfo::paths_pieces (PtOptions.paths_pieces, paths_min_piece)
  // Uniform grids over the leaf boxes (pt::build_grid; SceneTables::grid_*), large scenes where one beats the BVH scan: setup()
  // uploads the candidates of pt::build_scene_tables, choose_traversal() times them, keeps the fastest and frees the rest.
  struct DeviceGrid {
    pt::GridShape shape;
    size_t guard;  // empty cells in front of (and behind) the cell table proper
    const uint32_t* d_start;
    const ptd::Node* d_items;
    const ptd::Node* d_items_b;  // == d_items unless the build wants centre / half extent
    size_t bytes;
    std::vector<uint32_t> start;  // the host copy of what d_start holds, guard cells included (pt_stage_grid_info)
    size_t items = 0;             // records in d_items (a camera move reuses the buffers while the sizes stay)
    bool start_stale = false;     // a device build wrote d_start: `start` has its size but not yet its contents (grid_start_host fetches them)
  };
  std::vector<DeviceGrid> grids;
  size_t grid_pick = 0;  // grids[grid_pick] is the one the kernels walk (when grids is not empty)
  int tight_leaves = 0;  // sphere leaves with a tightened traversal box (pt::tighten_sphere_leaves)
  bool grid_enabled = true;      // the outcome of choose_traversal()
  int cap_bpc = 8;
  bool legacy = false;
  int debug_flags = 0;
  int record_form = 0;  // BatchInfo::split_records of the last batch (PtStats.record_form)
  int gather_form = 0;  // pt_sched.h GatherPlan::reported of the last batch (PtStats.gather_form)
  bool fuse_primary = true, fuse_bounces = true;
  bool aa_jitter = false;
};

// The objects' motion as a history sees it (PT_HISTORY_MOTION): the geoms its K is aligned to, and the motion table of the last lookup
// that found a geom moved.  A context holds one for its tile's K, a group (pt_group.cpp) one for the frame's; the device table belongs
// to the context that built it (history_motion_table in pt_post.cpp).
struct PtHistoryMotion {
  std::vector<PtGeom> geoms;     // the kept geoms, taken by a capture
  bool geoms_stale = true;       // pt_ctx_set_geoms has run since `geoms` was copied (or nothing was copied yet)
  void* d_table = nullptr;       // pthi::kMotionRow floats per geom, then one kind byte per geom
  std::vector<float> table;      // what d_table holds
  std::vector<uint8_t> kind;
  bool fresh = false;            // the table is that of `geoms` and the current geoms as they stand; moved: some kind != 0
  bool moved = false;
};

// The materials as a history sees them (PT_HISTORY_MATERIALS): the materials its K was rendered with, and the recolour table of the
// last lookup that found a material changed (history_recolor_table in pt_post.cpp).
struct PtHistoryMaterials {
  std::vector<PtMaterial> materials;  // the kept materials, taken by a capture
  bool stale = true;             // pt_ctx_set_materials has run since `materials` was copied (or nothing was copied yet)
  void* d_table = nullptr;       // pthi::kRecolorRow floats per geom, then one kind byte per geom
  std::vector<float> table;      // what d_table holds
  std::vector<uint8_t> kind;
  bool fresh = false;            // the table is that of `materials` and the current materials as they stand; changed: some kind != 0
  bool changed = false;
};

// One renderer instance = one device, one stream, one tile of the framebuffer.  The reference keeps this state in
// file-scope statics (pathtrace.cu:446-456); here it is an object so that one process can drive several GPUs
// (pt_group_*, pt_group.cpp) — the old single-instance entry points act on a default context.
struct PtContext : PtShared {
  // tile / batch geometry
  int N = 0, pixel_begin = 0, K = 1;
  int slot_shift = 0;  // BatchInfo::slot_shift
  int stripe = 0, stripe_stride = 0;
  int grid = 0;  // widest persistent grid (stats / test stages)
  int grid_gen = 0, grid_isect = 0, grid_shade = 0;
  ptd::Queues qs{};
  int64_t stride = 0;  // plane stride = Q*cap
  // device memory
  std::vector<void*> allocs;
  int64_t device_bytes = 0;
  float probe_ms[2] = {0.f, 0.f};  // a few iterations with the BVH scan / with the (fastest) grid, as timed by choose_traversal()
  int grid_primary = 0, grid_paths = 0;
  ptd::PathBuf buf[2]{};
  ptd::HitBuf hits{};
  ptd::RetireBuf ret{};  // retirement records + fill levels (pt_device.h)
  // The second record plane and the batch whose stream gather waits for the next batch's k_paths (pt_sched.h gather_plan).  Set and
  // consumed inside one pt_ctx_render call: nothing waits when a call returns.
  ptd::Word4* rec_plane1 = nullptr;  // as large as ret.rec (plane 0); absent where the form cannot apply or the allocation failed
  struct WaitingGather {
    bool live = false;
    ptk::BatchInfo b{};
    int plane = 0;  // where that batch's k_paths stored its records
  } waiting;
  int64_t inline_gathers = 0;  // batches gathered inside the next batch's k_paths (PtStats.inline_gathers)
  float* d_image = nullptr;
  // First-hit feature buffers (pt_ctx_render_features): PT_FEATURE_PLANES planes of N float4 sums; absent until the first feature pass
  float4* d_feat = nullptr;
  int grid_features = 0;
  void* d_denoise = nullptr;  // workspace of pt_ctx_denoise (pt_denoise_workspace_bytes(N)); absent until the first denoise call
  // Noise estimate (pt_ctx_noise_fold, csrc/pt_noise.hip): planes, partial sums and their sum (pt_noise_state_bytes(N)); absent until the first fold
  void* d_noise = nullptr;
  int noise_groups = 0;      // M: folds since pt_init / pt_clear that had something to fold
  int64_t noise_iters = 0;   // T: iterations those folds took
  int64_t rendered = 0;      // iterations handed to pt_ctx_render since pt_init / pt_clear (samples is zeroed by pt_reset_stats; setup()'s timing batches never count)
  // Convergence metric (PtOptions.convergence, pt_kernels.h ConvInfo): all of it absent when the option is 0
  int conv = 0;                // the option: N > 0 capture the frame at iteration N, -1 supplied
  bool conv_live = false;      // off while setup() renders its timing batches: they leave no trace in the curve or the frame
  bool conv_have_ref = false;  // d_ref holds the frame (supplied, or the batch that captures it has been submitted)
  int conv_last = 0;           // highest iteration submitted with the metric on
  float* d_ref = nullptr;      // [N][3]
  double* d_partial = nullptr;  // [K][Q][kConvWaves]
  double* d_sse = nullptr;      // [PT_CONVERGENCE_CAPACITY], iteration i at i - 1; all bits set (a NaN) = no value
  uint8_t* d_rgb8 = nullptr;  // lazily allocated output of pt_ctx_save_u8
  int32_t* d_cnt = nullptr;
  unsigned long long* d_stats = nullptr;
  // timing
  bool time_kernels = false;
  std::vector<EventPair> free_events, pending_isect, pending_render;
  double isect_ms = 0, render_ms = 0;
  int64_t isect_launches = 0;
  int64_t samples = 0;
  // Depth 0 once per camera (pt_sched.h batch_form): what the first-hit records now in buf[1], ret.rec and ret.sub were traced for —
  // every argument of the k_primary launch that wrote them but the batch's first iteration and its length, which that output does not
  // depend on.  run_batch launches k_primary again unless the next batch's arguments are these, bit for bit; what changes behind
  // the pointers they hold (the tables of a moved camera, a worker's pixel list, buffers armed again) clears primary_valid itself.
  struct PrimaryKey {
    ptk::SceneTables sc;
    ptd::Camera cam;
    ptk::BatchInfo b;  // iter_first = K = 0
    ptd::Queues qs;
    ptd::PathBuf out;
    ptd::RetireBuf ret;
    const void* kernels;
    int32_t grid, debug_flags;
  };
  PrimaryKey primary_key{};
  bool primary_valid = false;
  int64_t primary_launches = 0;  // k_primary launches of pt_render and the adaptive rounds (PtStats.primary_launches)
  // A batch that failed half-way (a launch or an event call returned an error) leaves counters and record regions in an
  // undefined state: the context refuses further renders instead of appending past them.
  bool failed = false;
  // Adaptive sampling (pt_ctx_adaptive_round, csrc/pt_adaptive.hip): all of it absent until the first round (d_list and the worker: or
  // until pt_stage_render_list)
  int opt_iters_per_batch = 0, opt_num_queues = 0;  // PtOptions, as given: a worker plans its own batches from them
  bool borrowed = false;           // a worker context: what PtShared holds belongs to its parent
  const int32_t* list = nullptr;   // BatchInfo::list of this context's batches (a worker's: the parent's d_list, or its d_list_frame)
  PtContext* worker = nullptr;     // the context that renders the pixel list; its tile is the list's m pixels, its d_image the group sum Sw
  int capacity = 0;                // a worker: the pixels it was planned and allocated for; its N is the LIVE list length, <= capacity
  int32_t* d_list = nullptr;       // N entries, the first worker->N in use
  int32_t* d_list_frame = nullptr; // a striped tile: the same entries as offsets in the frame, what the worker's batches read (pt_adaptive_round_list)
  void* d_acnt = nullptr;          // the plane cnt: N * ptad::Cnt
  void* d_select = nullptr;        // pt_adaptive_select_bytes(N)
  float* d_resolved = nullptr;     // [N][3], output of pt_ctx_resolve_device; absent until the first resolve
  // Reprojected sample history (pt_ctx_history_capture, csrc/pt_history.hip): all of it absent until the first capture
  void* d_hist = nullptr;          // pt_history_state_bytes(N): the kept planes K0 K1 K2, then the current plane C
  uint8_t* d_hist_reject = nullptr;  // one byte per geom: its material reflects (the first pt_ctx_history_reproject builds it)
  PtCamera hist_cam{};             // the camera K is aligned to
  bool hist_kept = false;          // K holds a capture (pt_ctx_history_drop forgets it)
  bool hist_current = false;       // C holds a reprojection for the current camera; pt_clear and a camera move make it absent
  void* d_hist_var = nullptr;      // pt_history_variance_bytes(N): VK, then VC; absent until the first capture with PT_HISTORY_VARIANCE or _MOMENTS
  uint32_t hist_var_kept = 0;      // the flag of the capture VK belongs to K0 by: the variance of K0 or its moments (0: a plain capture, K "kept without")
  uint32_t hist_var_current = 0;   // the flag of the lookup VC belongs to C by; 0 (absent) whenever C is
  // The feedback (PT_HISTORY_FEEDBACK): absent until the first call that carries the flag.  Three planes whose roles rotate: a capture
  // with the flag promotes the pending plane to FK by swapping two of these indices, it moves no bytes.
  void* d_hist_fb = nullptr;       // pt_history_feedback_bytes(N): three planes of N float4
  int fb_plane_kept = 0, fb_plane_current = 1, fb_plane_pending = 2;  // which plane holds FK, FC and P
  bool fb_kept = false;            // FK belongs to K (a capture without the flag leaves K "kept without feedback")
  bool fb_current = false;         // FC belongs to C; absent whenever C is
  bool fb_pending = false;         // P holds the tap of pt_history_denoise_feedback for the image as it stands
  int fb_keep_albedo = 0;          // the keep_albedo the last tap was made with: the unit of P.w, and of FK.w / FC.w after it
  // The objects' motion (PT_HISTORY_MOTION): the geoms K is aligned to beside hist_cam, and the motion table of the last lookup that
  // found a geom moved (absent until then): pthi::kMotionRow floats per geom, then one kind byte per geom
  PtHistoryMotion hist_motion;
  // The materials' edits (PT_HISTORY_MATERIALS): the materials K was rendered with, and the recolour table of the last lookup that
  // found one changed (absent until then)
  PtHistoryMaterials hist_materials;
  // The noise estimate of the blend (pt_ctx_history_noise): absent until the first estimate
  void* d_hist_noise = nullptr;    // pt_history_noise_bytes(N): the partial sums, SSE_blend, then the plane W
  bool hist_noise = false;         // W holds an estimate of the image as it stood; pt_clear and a move make it absent
  float* d_hist_ne = nullptr;      // the plane NE beside W (pt_ctx_history_noise_adaptive, pt_ctx_history_round_threshold): N floats; absent until the first of those
  bool hist_ne = false;            // NE belongs to the W that is present: pass A of those calls wrote both; absent whenever W is
  // The history round (pt_ctx_history_round): all of it absent until the first round that renders something
  float* d_hist_extra = nullptr;   // the extra plane E: N floats, the samples the image holds per pixel beyond the uniform ones
  bool hist_extra = false;         // E is present: from a round that rendered to pt_clear or a camera move, which zero it
  uint8_t* d_hist_emitter = nullptr;  // one byte per geom: its material emits (the first round builds it)
  // The history probes (pt_ctx_history_probe_keep / _check): all of it absent until the first keep (d_probe) or check (the rest)
  void* d_probe = nullptr;         // PK: 16 B per probe, for the probes of phase 0 (the most of any phase)
  float* d_probe_lam = nullptr;    // L: one float per probe (as many as PK), then the two counts {changed, skipped} as int32
  uint8_t* d_probe_moved = nullptr;  // one byte per geom: its matrices differ from the kept geoms', or its material from the kept materials'
  std::vector<uint8_t> probe_moved_dev;  // what d_probe_moved holds
  bool probe_kept = false;         // PK holds probes (pt_ctx_history_drop forgets them)
  int probe_first = 0, probe_iters = 0, probe_phase = 0;  // the iterations S held at the keep, and the probes' phase
  int probe_N = 0, probe_begin = 0;  // the tile they were kept for
  PtCamera probe_cam{};            // the camera at the keep
  std::vector<PtGeom> probe_geoms;  // the geoms at the keep
  bool probe_geoms_stale = true;   // pt_ctx_set_geoms has run since probe_geoms was copied (or nothing was copied yet)
  bool probe_geoms_changed = false;  // pt_ctx_set_geoms has run since the keep
  std::vector<PtMaterial> probe_materials;  // the materials at the keep
  bool probe_materials_stale = true;     // pt_ctx_set_materials has run since probe_materials was copied (or nothing was copied yet)
  bool probe_materials_changed = false;  // pt_ctx_set_materials has run since the keep
  bool probe_checked = false;      // L is the check of these probes against the C that is present
  bool probe_applied = false;      // a check has been applied to this C (the next lookup clears it)
  bool feat_fresh = false;         // a feature pass has run since pt_init / pt_clear / the last camera move
  // Moving the camera (pt_ctx_set_camera): the camera-independent tables on the host, and the grid to rebuild (the one init kept)
  pt::CameraBase camera_base;
  pt::GridRequest grid_request;
  PtSetupTimes setup_times{};
  // The device build of those tables (pt_ctx_set_camera_ex, csrc/pt_camera_tables.hip): camera_base on the device and the build's workspace,
  // all of it absent until the first move that asks for the device path
  struct DeviceBase {
    bool ready = false;
    const ptd::Node* nodes = nullptr;
    const ptd::TopEntry* top = nullptr;
    const ptct::DeviceGeom* geoms = nullptr;
    ptct::BuildRecord* rec = nullptr;
    uint32_t* count = nullptr;    // one word per cell of grid_request's resolution: the counters, then the scatter's fill levels
    uint32_t* sums = nullptr;     // the scan's sums per workgroup
    uint32_t* scratch = nullptr;  // the scatter's list: scratch_cap leaf indices
    size_t scratch_cap = 0;
  };
  DeviceBase device_base;
  PtSetCameraTimes camera_times{};  // the last move (pt_get_set_camera_times)
  PtSetGeomsTimes geoms_times{};    // the last pt_ctx_set_geoms (pt_get_set_geoms_times)
  // Editing the materials (pt_ctx_set_materials): the PtMaterials the device table was made from, kept from pt_init on (44 B each)
  std::vector<PtMaterial> materials;
  PtSetMaterialsTimes materials_times{};  // the last pt_ctx_set_materials (pt_get_set_materials_times)
  bool hist_reject_stale = false, hist_emitter_stale = false;  // pt_ctx_set_materials has run since d_hist_reject / d_hist_emitter was built
  bool adaptive = false;           // the adaptive state: from the first round to pt_clear
  int adaptive_rounds = 0;
  int64_t adaptive_last = 0;       // highest iteration number folded or merged
};

// What a group (pt_group.cpp) asks of its contexts beyond the C ABI; C++ linkage, so none of it is exported under a plain name.
struct PtCtxState {
  bool adaptive;     // in the adaptive state
  int groups;        // M: groups folded
  int64_t iters;     // T: iterations those folds took
  int64_t unfolded;  // iterations rendered since the last fold
};
PtCtxState pt_ctx_state(const PtContext* c);
// the refusal, under the name `who`, of a context whose batch failed half-way, and (uniform) of one in the adaptive state
int pt_ctx_admit_state(const PtContext* c, const char* who, bool uniform);
// What pt_adaptive_round_threshold refuses before its threshold, in its order and under the name `who`, apart from a tile that is not
// whole contiguous rows; folds == false: apart from the state of the folds too (pt_render_threshold's first look).
int pt_ctx_adaptive_refusal(const PtContext* c, const char* who, int iter_first, int group_iters, float max_fraction, bool folds);
int pt_ctx_camera_refusal(const PtContext* c, const PtCamera* cam, const char* who);  // what pt_set_camera refuses, in its order; nothing changes
int pt_ctx_geoms_refusal(const PtContext* c, const PtGeom* geoms, int num_geoms, const char* who);  // what pt_set_geoms refuses, in its order; nothing changes
int pt_ctx_materials_refusal(const PtContext* c, const PtMaterial* materials, int num_materials, const char* who);  // what pt_set_materials refuses, in its order; nothing changes
int pt_ctx_camera_refusal_ex(const PtContext* c, const PtCamera* cam, uint32_t flags, const char* who);  // ... with the undefined flag bit after the null camera
int pt_ctx_enter_adaptive(PtContext* c);  // the count plane with the fold's (T, M) in every pixel, unless the context is in the adaptive state already
// The history of a group (pt_group_history_*): the frame's K, C, VK and VC live with the group; a context is asked for what only it knows.
int pt_ctx_admit_no_extras(const PtContext* c, const char* who);  // the refusal of a context that holds the extra plane E (what reads a uniform SUM)
bool pt_ctx_features_fresh(const PtContext* c);                   // a feature pass has run since the last clear or move
bool pt_ctx_history_extra_present(const PtContext* c);            // E is present
const float* pt_ctx_device_history_extra(PtContext* c);           // E of the tile on the device, nullptr while absent
int pt_history_check_flags(const char* who, uint32_t flags, bool motion);  // the flag word of pt_history_capture_ex / (motion) _reproject_ex
int pt_history_check_denoise_flags(const char* who, uint32_t flags);       // the flag word of pt_history_denoise_ex
// What pt_history_round refuses before its options, in its order and under the name `who`, apart from a tile that is not whole rows.
int pt_ctx_history_round_refusal(const PtContext* c, const char* who, int iter_first, int group_iters);
// The per-geom tables of a history on the context's device, built at first use and kept by the context: reject_geom (the lookup) or
// emitter_geom (the round's key); *num_geoms the geoms of the scene.  Blocking the first time.
int pt_ctx_history_geom_table(PtContext* c, bool emitter, const uint8_t** table_dev, int* num_geoms);
// The motion table of `m`'s kept geoms against the context's current ones, on the context's device: *table_dev and *kind_dev, both
// nullptr when no geom moved (nothing allocated or uploaded then).
int pt_ctx_history_motion_table(PtContext* c, PtHistoryMotion* m, const float** table_dev, const uint8_t** kind_dev);
const std::vector<PtGeom>& pt_ctx_geoms(const PtContext* c);  // the geoms as they stand
const PtCamera& pt_ctx_camera(const PtContext* c);            // the camera as it stands

namespace ptc {
using Ctx = PtContext;

PtContext* default_context();  // the instance behind pt_init / pt_render / pt_free, or nullptr

template <typename T>
int dalloc(Ctx& g, T** out, size_t count) {  // owned by the context: destroy() frees it
  void* p = nullptr;
  size_t bytes = std::max<size_t>(count * sizeof(T), 16);
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) return pt_fail("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
  g.allocs.push_back(p);
  g.device_bytes += (int64_t)bytes;
  *out = reinterpret_cast<T*>(p);
  return 0;
}
// A buffer that exists from its first use on: `bytes` through dalloc if `p` is still null, then zeroed as `zero` says or left as it comes.
enum class Zero { none, blocking, on_stream };
template <typename T>
int ensure(Ctx& g, T*& p, size_t bytes, Zero zero = Zero::none) {
  if (p) return 0;
  char* q = nullptr;
  if (dalloc(g, &q, bytes)) return -1;
  p = reinterpret_cast<T*>(q);
  if (zero == Zero::blocking) HIP_OK(hipMemset(q, 0, bytes));
  if (zero == Zero::on_stream) HIP_OK(hipMemsetAsync(q, 0, bytes, g.stream));
  return 0;
}
struct Scratch {  // frees on scope exit
  std::vector<void*> p;
  ~Scratch() { for (void* q : p) (void)hipFree(q); }
  template <typename T>
  T* get(size_t n) {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(n * sizeof(T), 16)) != hipSuccess) return nullptr;
    p.push_back(q);
    return reinterpret_cast<T*>(q);
  }
};

int need(const PtContext* c, const char* who);  // the context exists, or the refusal under the public name `who`
// The rest of an entry point's prologue: the requirements in `req`, checked in the order of the enumerators; the first one not met is
// the refusal, 0 when all hold.  An entry point whose own checks lie between two of them, or that orders them differently, calls
// admit() once per run of requirements: the order of an entry point's refusals is its behaviour.
enum Require : unsigned {
  kNotFailed = 1,   // no batch of the context failed half-way
  kUniform = 2,     // not in the adaptive state
  kWholeRows = 4,   // the tile is rows of the image, whole and one after the other
  kFoldedAll = 8,   // nothing rendered since the last fold
  kOnDevice = 16,   // not a refusal: makes the context's device current
  kNoExtras = 32,   // the history round's extra plane is absent (checked right after kUniform: both say "one sample count describes the image")
};
int admit(const PtContext& g, const char* who, unsigned req);

// The host form of an entry point: refuses a null buffer, has `source` name the device buffer (the `_device` form of the entry point,
// or a readback's own check; nonzero: refused), copies per_pixel * N elements of it to `host` on the context's stream and synchronises.
template <typename T, typename Source>
int copy_out(PtContext* c, const char* who, T* host, size_t per_pixel, Source source, hipMemcpyKind kind = hipMemcpyDeviceToHost) {
  if (!host) return pt_fail("%s: null buffer", who);
  const T* d = nullptr;
  if (source(&d)) return -1;
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipMemcpyAsync(host, d, per_pixel * (size_t)c->N * sizeof(T), kind, c->stream));
  return pt_ctx_sync(c);
}

// pt_api.cpp
ptk::SceneTables tables(const Ctx& g);
ptk::BatchInfo tile_batch(const Ctx& g, int iter_first, int K);  // BatchInfo's iterations and the fields that describe the tile
int run_batch(Ctx& g, int iter_first, int kb, int after = 0);  // after: batches of the same render call that follow this one
int batch_iters_for(int iters_per_batch, int N, int* slot_shift);
int plan_batches(Ctx& g, const PtOptions& opt);
void plan_launch(Ctx& g);
int grid_start_host(Ctx& g, Ctx::DeviceGrid& d);  // d.start as d_start holds it (fetched after a device build of the tables)
int alloc_batch_buffers(Ctx& g);
int get_events(Ctx& g, EventPair* ev);
ptd::Queues single_queue(const Ctx& g, int n);
void destroy(Ctx* c);
// pt_post.cpp: the worker context of adaptive sampling
int ensure_worker(Ctx& g, int capacity);                  // g.worker: a context planned for `capacity` pixels, its live tile the first `capacity` entries of g.d_list
void set_worker_live(Ctx& w, int m);                      // the worker's tile := the first m <= capacity entries; nothing allocated, freed or cleared
int render_list(Ctx& g, int iter_first, int iter_count);  // those iterations of the listed pixels into the worker's cleared sum
}  // namespace ptc
