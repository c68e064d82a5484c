// pt_group.cpp — one process, several MI355X: BASELINE config 4 (framebuffer tiled across the GPUs of a node, a
// single RCCL gather over xGMI at image write-out; SURVEY.md §8e, §5 "Distributed communication backend").
//
// The reference is single-device (src/preview.cpp:112 cudaGLSetGLDevice(0)); its write-out point is saveImage()
// (src/main.cpp:86-107).  Here every device owns the rows i, i+n, i+2n, ... of the frame (work per row varies
// smoothly down the cornell frame, interleaving gives every device the same mix) and runs ALL iterations on them
// on its own stream; samples are keyed by the global pixel index (makeSeededRandomEngine(iter, idx, depth),
// src/pathtrace.cu:203-207,368), so nothing is ever summed across devices and the assembled image is bit-identical
// to the single-GPU image.  The only communication is, once per write-out, one grouped ncclSend/ncclRecv of the
// tiles into devices[0] on a ncclCommInitAll communicator — xGMI is point-to-point, the tiles go straight to the
// root over their own links, there is no ring and no reduction.  Placement of the interleaved rows (a strided 2-D
// copy on the root device) and one D2H copy follow.
//
// Two transports for that one exchange (PtGroup::transport, pt_group_create_ex):
//   RCCL  the grouped ncclSend / ncclRecv above — the default for distinct devices;
//   COPY  hipMemcpyPeerAsync (hipMemcpyAsync when source and root are the same device) of every tile into the same
//         receive buffer at the same offsets, ordered after the tile's producer by an event the root's stream waits
//         on.  RCCL cannot put two ranks of one communicator on one device, so this is what a group whose device
//         list names a device more than once (e.g. {0, 0, 0}: several contexts, one GPU) uses automatically; it
//         makes the whole multi-context path — per-context streams, receive offsets, strided row placement,
//         preview exchange — testable on a one-GPU box, and is a fallback where RCCL is unwanted.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "pt_adaptive.h"
#include "pt_context.h"  // HIP_OK; a group reaches its contexts through the C ABI and the helpers declared there
#include "pt_denoise.h"
#include "pt_group_select.h"
#define NCCL_OK(expr)                                                                                      \
  do {                                                                                                     \
    ncclResult_t r_ = (expr);                                                                              \
    if (r_ != ncclSuccess) return pt_fail("%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__); \
  } while (0)

struct PtGroup {
  int W = 0, H = 0, n = 0;
  int transport = PT_GROUP_TRANSPORT_RCCL;  // resolved (never AUTO) after pt_group_create_ex
  std::vector<hipEvent_t> ready;            // COPY transport: "tile i is complete" (recorded on context i's stream)
  std::vector<int> devices;
  std::vector<PtContext*> ctx;
  std::vector<ncclComm_t> comms;
  std::vector<int> rows;         // image rows owned by device i
  std::vector<size_t> recv_off;  // pixel offset of device i's tile in the root's receive buffer (i >= 1)
  size_t recv_pixels = 0;
  float* d_recv = nullptr;    // root: tiles of devices 1..n-1, float RGB
  float* d_full = nullptr;    // root: assembled frame
  uint8_t* d_recv8 = nullptr; // same for the converted bytes (3 B/pixel)
  uint8_t* d_full8 = nullptr;
  std::vector<uint8_t*> d_prev;  // per device: RGBA8 preview of its tile (sendImageToPBO)
  uint8_t* d_recv_prev = nullptr;  // root: preview tiles of devices 1..n-1 / assembled preview (kept: previews recur)
  uint8_t* d_full_prev = nullptr;
  float* d_recv_feat = nullptr;  // root: one feature plane of the tiles of devices 1..n-1 (16 B per pixel) / the assembled planes
  float* d_full_feat = nullptr;
  float* d_full_noise = nullptr;  // root: the assembled noise planes (pt_group_denoise_guided; the receive buffer is d_recv_feat)
  void* d_denoise = nullptr;  // root: workspace of pt_group_denoise over the whole frame
  // Adaptive sampling by threshold (pt_group_adaptive_round_threshold); all of it absent until the first round (the pair buffers: or
  // until the first write-out of the count planes)
  std::vector<void*> d_pack;       // per context, on its device: {w_p, T_p} of its tile, 8 B per pixel
  std::vector<int32_t*> d_part;    // per context i >= 1, on its device: its part of the frame's list
  int32_t* d_recv_pair = nullptr;  // root: 8 B per pixel of the tiles of devices 1..n-1 (the packed pairs; the count planes at write-out)
  int32_t* d_full_pair = nullptr;  // root: the same of the assembled frame
  void* d_select = nullptr;        // root: the selection's workspace for W*H pixels (pt_adaptive_select_bytes)
  void* d_partition = nullptr;     // root: the partition's workspace (pt_group_partition_bytes)
  int32_t* d_list = nullptr;       // root: the frame's list, W*H entries, the first m in use
  int32_t* d_parts = nullptr;      // root: the contexts' lists back to back
  uint32_t* d_result = nullptr;    // root: above, m, m_0 .. m_(n-1)
  hipEvent_t parts_ready = nullptr;  // root: the parts are complete (recorded on the root's stream)
};

namespace {

void release(PtGroup* g) {
  if (!g) return;
  for (size_t i = 0; i < g->comms.size(); ++i)
    if (g->comms[i]) {
      (void)hipSetDevice(g->devices[i]);
      (void)ncclCommDestroy(g->comms[i]);
    }
  for (size_t i = 0; i < g->ready.size(); ++i)
    if (g->ready[i]) {
      (void)hipSetDevice(g->devices[i]);
      (void)hipEventDestroy(g->ready[i]);
    }
  if (!g->devices.empty()) (void)hipSetDevice(g->devices[0]);
  for (void* p : {(void*)g->d_recv, (void*)g->d_full, (void*)g->d_recv8, (void*)g->d_full8, (void*)g->d_recv_prev,
                  (void*)g->d_full_prev, (void*)g->d_recv_feat, (void*)g->d_full_feat, (void*)g->d_full_noise, g->d_denoise, (void*)g->d_recv_pair,
                  (void*)g->d_full_pair, g->d_select, g->d_partition, (void*)g->d_list, (void*)g->d_parts, (void*)g->d_result})
    if (p) (void)hipFree(p);
  if (g->parts_ready) (void)hipEventDestroy(g->parts_ready);
  for (size_t i = 0; i < g->d_pack.size() || i < g->d_part.size(); ++i) {
    (void)hipSetDevice(g->devices[i]);
    if (i < g->d_pack.size() && g->d_pack[i]) (void)hipFree(g->d_pack[i]);
    if (i < g->d_part.size() && g->d_part[i]) (void)hipFree(g->d_part[i]);
  }
  for (size_t i = 0; i < g->d_prev.size(); ++i)
    if (g->d_prev[i]) {
      (void)hipSetDevice(g->devices[i]);
      (void)hipFree(g->d_prev[i]);
    }
  for (PtContext* c : g->ctx) (void)pt_ctx_destroy(c);
  delete g;
}

// COPY transport: the root's stream waits for tile i's producer, then pulls the tile into the receive buffer.
int exchange_copy(PtGroup* g, size_t bytes_per_pixel, char* root_recv, const void* const* src) {
  hipStream_t root = (hipStream_t)pt_ctx_stream(g->ctx[0]);
  for (int i = 1; i < g->n; ++i) {
    const size_t bytes = bytes_per_pixel * (size_t)pt_ctx_pixel_count(g->ctx[i]);
    HIP_OK(hipSetDevice(g->devices[i]));
    HIP_OK(hipEventRecord(g->ready[i], (hipStream_t)pt_ctx_stream(g->ctx[i])));
    HIP_OK(hipSetDevice(g->devices[0]));
    HIP_OK(hipStreamWaitEvent(root, g->ready[i], 0));
    char* dst = root_recv + bytes_per_pixel * g->recv_off[i];
    if (g->devices[i] == g->devices[0]) HIP_OK(hipMemcpyAsync(dst, src[i], bytes, hipMemcpyDeviceToDevice, root));
    else HIP_OK(hipMemcpyPeerAsync(dst, g->devices[0], src[i], g->devices[i], bytes, root));
  }
  return 0;
}

// The one exchange of a write-out: device i >= 1 hands `elems_per_pixel * pixels_i` elements of `src(i)` to the root,
// which receives them back to back (recv_off) on its stream.  RCCL: one grouped send/recv, each send on its own
// device's stream.
template <typename T, typename SrcFn>
int exchange(PtGroup* g, ncclDataType_t type, int elems_per_pixel, T* root_recv, SrcFn src) {
  if (g->n == 1) return 0;
  if (g->transport == PT_GROUP_TRANSPORT_COPY) {
    std::vector<const void*> srcs(g->n, nullptr);
    for (int i = 1; i < g->n; ++i) srcs[i] = src(i);
    return exchange_copy(g, sizeof(T) * (size_t)elems_per_pixel, reinterpret_cast<char*>(root_recv), srcs.data());
  }
  NCCL_OK(ncclGroupStart());
  int rc = 0;
  for (int i = 1; i < g->n && !rc; ++i) {  // an error inside the group must still close it
    const size_t count = (size_t)elems_per_pixel * pt_ctx_pixel_count(g->ctx[i]);
    ncclResult_t r = ncclSuccess;
    if (hipSetDevice(g->devices[i]) != hipSuccess) rc = pt_fail("hipSetDevice(%d) failed", g->devices[i]);
    else if ((r = ncclSend(src(i), count, type, 0, g->comms[i], (hipStream_t)pt_ctx_stream(g->ctx[i]))) != ncclSuccess)
      rc = pt_fail("ncclSend from device %d failed: %s", g->devices[i], ncclGetErrorString(r));
    else if (hipSetDevice(g->devices[0]) != hipSuccess) rc = pt_fail("hipSetDevice(%d) failed", g->devices[0]);
    else if ((r = ncclRecv(root_recv + (size_t)elems_per_pixel * g->recv_off[i], count, type, i, g->comms[0],
                           (hipStream_t)pt_ctx_stream(g->ctx[0]))) != ncclSuccess)
      rc = pt_fail("ncclRecv from device %d failed: %s", g->devices[i], ncclGetErrorString(r));
  }
  const ncclResult_t e = ncclGroupEnd();
  if (!rc && e != ncclSuccess) rc = pt_fail("ncclGroupEnd failed: %s", ncclGetErrorString(e));
  return rc;
}

// After a failed exchange / placement some sends, receives or copies may already be queued on the devices' streams:
// drain them (ignoring further errors, keeping the first message) before the caller sees the failure.
int fail_after_drain(PtGroup* g) {
  const std::string first = pt_last_error();
  for (PtContext* c : g->ctx) (void)pt_ctx_sync(c);
  return pt_fail("%s", first.c_str());
}

// Rows of device i (tile order) -> rows i, i+n, ... of the frame, on the root's stream.
template <typename T>
int place_rows(PtGroup* g, int i, const T* tile, T* full, size_t bytes_per_pixel) {
  const size_t row = (size_t)g->W * bytes_per_pixel;
  HIP_OK(hipMemcpy2DAsync(reinterpret_cast<char*>(full) + (size_t)i * row, (size_t)g->n * row, tile, row, row, (size_t)g->rows[i],
                          hipMemcpyDeviceToDevice, (hipStream_t)pt_ctx_stream(g->ctx[0])));
  return 0;
}

// The device side of the two write-out gathers (n > 1; the root device is current), on the root's stream: the tiles' exchange into
// the receive buffer and the placement of everybody's rows in the frame buffer.  What follows — a copy to the host, the filter —
// is queued behind them on the same stream.
int assemble_image(PtGroup* g) {  // -> g->d_full: W*H*3 floats
  const size_t frame = (size_t)g->W * g->H;
  if (!g->d_full) HIP_OK(hipMalloc((void**)&g->d_full, frame * 12));
  if (!g->d_recv) HIP_OK(hipMalloc((void**)&g->d_recv, g->recv_pixels * 12));
  if (exchange(g, ncclFloat, 3, g->d_recv, [&](int i) { return pt_ctx_device_image(g->ctx[i]); })) return fail_after_drain(g);
  HIP_OK(hipSetDevice(g->devices[0]));
  for (int i = 0; i < g->n; ++i)
    if (place_rows(g, i, i == 0 ? pt_ctx_device_image(g->ctx[0]) : g->d_recv + 3 * g->recv_off[i], g->d_full, 12))
      return fail_after_drain(g);
  return 0;
}
int need_features(PtGroup* g, const char* who) {
  for (PtContext* c : g->ctx)
    if (!pt_ctx_device_features(c)) return pt_fail("%s: no feature pass has been rendered (pt_group_render_features)", who);
  return 0;
}
// `count` float4 planes of every context (planes(c): plane 0 of context c, the planes contiguous) -> *full: the planes of the frame
template <typename PlanesFn>
int assemble_planes(PtGroup* g, int count, float** full, PlanesFn planes) {
  const size_t frame = (size_t)g->W * g->H;
  if (!*full) HIP_OK(hipMalloc((void**)full, count * frame * 16));
  if (!g->d_recv_feat) HIP_OK(hipMalloc((void**)&g->d_recv_feat, g->recv_pixels * 16));
  for (int pl = 0; pl < count; ++pl) {  // the root's stream orders plane pl + 1's receives behind plane pl's placement
    auto tile = [&](int i) { return planes(g->ctx[i]) + 4 * (size_t)pl * pt_ctx_pixel_count(g->ctx[i]); };
    if (exchange(g, ncclFloat, 4, g->d_recv_feat, tile)) return fail_after_drain(g);
    HIP_OK(hipSetDevice(g->devices[0]));
    for (int i = 0; i < g->n; ++i)
      if (place_rows(g, i, i == 0 ? tile(0) : g->d_recv_feat + 4 * g->recv_off[i], *full + 4 * pl * frame, 16)) return fail_after_drain(g);
  }
  return 0;
}
int assemble_features(PtGroup* g) {  // -> g->d_full_feat: PT_FEATURE_PLANES planes of W*H float4
  return assemble_planes(g, PT_FEATURE_PLANES, &g->d_full_feat, [](PtContext* c) { return pt_ctx_device_features(c); });
}
int assemble_noise(PtGroup* g) {  // -> g->d_full_noise: PT_NOISE_PLANES planes of W*H float4
  return assemble_planes(g, PT_NOISE_PLANES, &g->d_full_noise, [](PtContext* c) { return pt_ctx_device_noise(c); });
}

// 8 bytes per pixel of every context (the packed pairs of a round, the count planes at write-out) -> g->d_full_pair: the frame's
int assemble_pairs(PtGroup* g, const std::vector<const int32_t*>& tiles) {
  const size_t frame = (size_t)g->W * g->H;
  HIP_OK(hipSetDevice(g->devices[0]));
  if (!g->d_full_pair) HIP_OK(hipMalloc((void**)&g->d_full_pair, frame * 8));
  if (!g->d_recv_pair) HIP_OK(hipMalloc((void**)&g->d_recv_pair, g->recv_pixels * 8));
  if (exchange(g, ncclInt32, 2, g->d_recv_pair, [&](int i) { return tiles[i]; })) return fail_after_drain(g);
  HIP_OK(hipSetDevice(g->devices[0]));
  for (int i = 0; i < g->n; ++i)
    if (place_rows(g, i, i == 0 ? tiles[0] : g->d_recv_pair + 2 * g->recv_off[i], g->d_full_pair, 8)) return fail_after_drain(g);
  return 0;
}

// The contexts of a group share the fold counters M and T and the state they are in (pt_group_noise_fold and the group's rounds keep
// them so; pt_group_context lets a caller break it): the first context that differs from context 0 is the refusal.
int shared_state(PtGroup* g, const char* who, PtCtxState* out) {
  const PtCtxState s0 = pt_ctx_state(g->ctx[0]);
  for (int i = 1; i < g->n; ++i) {
    const PtCtxState s = pt_ctx_state(g->ctx[i]);
    if (s.groups != s0.groups || s.iters != s0.iters)
      return pt_fail("%s: context %d folded %d groups of %lld iterations, context 0 %d of %lld; the contexts of a group share them", who, i, s.groups,
                     (long long)s.iters, s0.groups, (long long)s0.iters);
    if (s.adaptive != s0.adaptive)
      return pt_fail("%s: context %d is %s the adaptive state, context 0 %s it; the contexts of a group share it", who, i, s.adaptive ? "in" : "out of",
                     s0.adaptive ? "in" : "out of");
  }
  *out = s0;
  return 0;
}

// One round of pt_group_adaptive_round_threshold for n > 1, after the arguments' refusals; the driver's min_pixels as in the context's round.
//
// Buffer order.  The root writes d_list and d_parts on its own stream; context i reads its part on ITS stream.
//   COPY: context i's copy out of d_parts waits for parts_ready, recorded on the root's stream behind the partition.  The next
//         round's pack exchange has the root's stream wait for ready[i], recorded on context i's stream behind that copy (and behind the
//         render and merge that follow it), before the root selects and partitions again: the parts are never overwritten early.
//   RCCL: the sends of the parts are on the root's stream like the partition before them and the next round's selection after them.
//         Context i receives into its own d_part[i] on its stream, which also copies it into the context's list; the next receive
//         into d_part[i] is behind that copy in stream order.
// Either way the root's host thread has synchronised the root's stream in between (the read-back), and d_pack[i] is written by
// context i's stream only after the exchange that read it: COPY through that synchronise, RCCL because the send is on that stream.
int group_round(PtGroup* g, const char* who, int iter_first, int group_iters, float threshold, float max_fraction, int min_pixels, int* above, int* selected) {
  const int n = g->n, W = g->W, H = g->H;
  const size_t frame = (size_t)W * H;
  for (int i = 0; i < n; ++i)
    if (pt_ctx_adaptive_refusal(g->ctx[i], who, iter_first, group_iters, max_fraction, true)) return -1;
  if (pt_adaptive_check_threshold(who, threshold)) return -1;
  if (n > ptgs::kMaxParts || H >= 32768 || frame > ((size_t)1 << 30))
    return pt_fail("%s: %d contexts on a frame of %d x %d: at most %d contexts, fewer than 32768 rows, at most 2^30 pixels", who, n, W, H, ptgs::kMaxParts);
  PtCtxState shared{};
  if (shared_state(g, who, &shared)) return -1;
  const int cap = ptad::list_length((double)max_fraction, (int64_t)frame);
  hipStream_t root = (hipStream_t)pt_ctx_stream(g->ctx[0]);

  // the group's buffers: the first round
  HIP_OK(hipSetDevice(g->devices[0]));
  if (!g->d_select) HIP_OK(hipMalloc(&g->d_select, pt_adaptive_select_bytes(frame)));
  if (!g->d_partition) HIP_OK(hipMalloc(&g->d_partition, pt_group_partition_bytes(frame, n)));
  if (!g->d_list) HIP_OK(hipMalloc((void**)&g->d_list, frame * sizeof(int32_t)));
  if (!g->d_parts) HIP_OK(hipMalloc((void**)&g->d_parts, frame * sizeof(int32_t)));
  if (!g->d_result) HIP_OK(hipMalloc((void**)&g->d_result, (2 + (size_t)n) * sizeof(uint32_t)));
  if (!g->parts_ready) HIP_OK(hipEventCreateWithFlags(&g->parts_ready, hipEventDisableTiming));
  if (g->d_pack.empty()) g->d_pack.assign(n, nullptr), g->d_part.assign(n, nullptr);
  for (int i = 0; i < n; ++i) {
    const size_t pixels = (size_t)pt_ctx_pixel_count(g->ctx[i]);
    HIP_OK(hipSetDevice(g->devices[i]));
    if (!g->d_pack[i]) HIP_OK(hipMalloc(&g->d_pack[i], pixels * 8));
    if (i >= 1 && !g->d_part[i]) HIP_OK(hipMalloc((void**)&g->d_part[i], pixels * sizeof(int32_t)));
  }

  // collect on the root: every context packs on its own stream, one exchange, the rows into the frame, key, select, partition
  std::vector<const int32_t*> tiles(n, nullptr);
  for (int i = 0; i < n; ++i) {
    if (pt_ctx_enter_adaptive(g->ctx[i])) return -1;
    HIP_OK(hipSetDevice(g->devices[i]));
    if (pt_group_pack_launch((hipStream_t)pt_ctx_stream(g->ctx[i]), pt_ctx_pixel_count(g->ctx[i]), pt_ctx_device_noise(g->ctx[i]),
                             pt_ctx_device_counts(g->ctx[i]), g->d_pack[i]))
      return -1;
    tiles[i] = static_cast<const int32_t*>(g->d_pack[i]);
  }
  if (assemble_pairs(g, tiles)) return -1;
  if (pt_group_keys_launch(root, W, H, g->d_full_pair, pt_adaptive_select_keys(g->d_select, frame)) ||
      pt_adaptive_select_threshold_keys_launch(root, W, H, threshold, cap, g->d_select, g->d_list) ||
      pt_group_partition_launch(root, W, n, g->d_list, pt_adaptive_select_result(g->d_select, frame), cap, g->d_partition, g->d_parts, g->d_result))
    return fail_after_drain(g);

  // read back: above, m and the parts' lengths, 8 + 4n bytes and ONE synchronise
  std::vector<uint32_t> result(2 + (size_t)n, 0u);
  HIP_OK(hipMemcpyAsync(result.data(), g->d_result, result.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, root));
  HIP_OK(hipStreamSynchronize(root));
  const int m = (int)result[1];
  int64_t sum = 0;
  for (int i = 0; i < n; ++i) sum += result[2 + (size_t)i];
  bool fits = m >= 0 && m <= cap && (int)result[0] >= m && sum == m;
  for (int i = 0; i < n && fits; ++i) fits = (int64_t)result[2 + (size_t)i] <= pt_ctx_pixel_count(g->ctx[i]);
  if (!fits) return pt_fail("%s: the selection left %u above, a list of %u (cap %d) in parts that add up to %lld", who, result[0], result[1], cap, (long long)sum);
  const bool render = m > 0 && (int)result[0] > min_pixels;
  if (above) *above = (int)result[0];
  if (selected) *selected = render ? m : 0;
  if (!render) return 0;  // nothing rendered or merged, no context counts a round

  // distribute and render: part i to context i, on context i's stream
  HIP_OK(hipEventRecord(g->parts_ready, root));
  std::vector<const int32_t*> lists(n, nullptr);
  std::vector<size_t> off(n, 0);
  for (int i = 1; i < n; ++i) off[i] = off[i - 1] + result[2 + (size_t)i - 1];
  lists[0] = g->d_parts;
  if (g->transport == PT_GROUP_TRANSPORT_COPY) {
    for (int i = 1; i < n; ++i) {
      hipStream_t si = (hipStream_t)pt_ctx_stream(g->ctx[i]);
      const size_t bytes = (size_t)result[2 + (size_t)i] * sizeof(int32_t);
      HIP_OK(hipSetDevice(g->devices[i]));
      HIP_OK(hipStreamWaitEvent(si, g->parts_ready, 0));
      if (bytes && g->devices[i] == g->devices[0]) HIP_OK(hipMemcpyAsync(g->d_part[i], g->d_parts + off[i], bytes, hipMemcpyDeviceToDevice, si));
      else if (bytes) HIP_OK(hipMemcpyPeerAsync(g->d_part[i], g->devices[i], g->d_parts + off[i], g->devices[0], bytes, si));
      lists[i] = g->d_part[i];
    }
  } else {
    NCCL_OK(ncclGroupStart());
    int rc = 0;
    for (int i = 1; i < n && !rc; ++i) {  // an error inside the group must still close it
      const size_t count = result[2 + (size_t)i];
      lists[i] = g->d_part[i];
      if (!count) continue;
      ncclResult_t r = ncclSuccess;
      if (hipSetDevice(g->devices[0]) != hipSuccess) rc = pt_fail("hipSetDevice(%d) failed", g->devices[0]);
      else if ((r = ncclSend(g->d_parts + off[i], count, ncclInt32, i, g->comms[0], root)) != ncclSuccess)
        rc = pt_fail("ncclSend to device %d failed: %s", g->devices[i], ncclGetErrorString(r));
      else if (hipSetDevice(g->devices[i]) != hipSuccess) rc = pt_fail("hipSetDevice(%d) failed", g->devices[i]);
      else if ((r = ncclRecv(g->d_part[i], count, ncclInt32, 0, g->comms[i], (hipStream_t)pt_ctx_stream(g->ctx[i]))) != ncclSuccess)
        rc = pt_fail("ncclRecv on device %d failed: %s", g->devices[i], ncclGetErrorString(r));
    }
    const ncclResult_t e = ncclGroupEnd();
    if (!rc && e != ncclSuccess) rc = pt_fail("ncclGroupEnd failed: %s", ncclGetErrorString(e));
    if (rc) return fail_after_drain(g);
  }
  for (int i = 0; i < n; ++i) {  // asynchronous: the contexts render concurrently; a context without pixels counts the round
    const int pixels = pt_ctx_pixel_count(g->ctx[i]);
    if (pt_ctx_adaptive_round_list_device(g->ctx[i], iter_first, group_iters, lists[i], (int)result[2 + (size_t)i], cap < pixels ? cap : pixels))
      return fail_after_drain(g);
  }
  return 0;
}

}  // namespace

extern "C" {

int pt_group_create_ex(const PtSceneDesc* scene, const PtOptions* base, const int* devices, int num_devices, int transport,
                       PtGroup** out) {
  if (!out) return pt_fail("pt_group_create: null output");
  *out = nullptr;
  if (!scene || !devices || num_devices <= 0) return pt_fail("pt_group_create: bad argument");
  if (transport != PT_GROUP_TRANSPORT_AUTO && transport != PT_GROUP_TRANSPORT_RCCL && transport != PT_GROUP_TRANSPORT_COPY)
    return pt_fail("pt_group_create: unknown transport %d", transport);
  const int W = scene->camera.resolution[0], H = scene->camera.resolution[1];
  if (num_devices > H) return pt_fail("pt_group_create: more devices (%d) than image rows (%d)", num_devices, H);
  bool shared = false;  // a device named more than once: several contexts on one GPU
  for (int i = 0; i < num_devices; ++i)
    for (int j = 0; j < i; ++j) shared |= devices[i] == devices[j];
  if (shared && transport == PT_GROUP_TRANSPORT_RCCL)
    return pt_fail("pt_group_create: a device is listed twice; RCCL cannot place two ranks of one communicator on one "
                   "device (use PT_GROUP_TRANSPORT_AUTO or _COPY)");
  PtGroup* g = new PtGroup();
  g->W = W, g->H = H, g->n = num_devices;
  g->transport = transport == PT_GROUP_TRANSPORT_AUTO ? (shared ? PT_GROUP_TRANSPORT_COPY : PT_GROUP_TRANSPORT_RCCL) : transport;
  g->devices.assign(devices, devices + num_devices);
  g->rows.resize(num_devices);
  g->recv_off.assign(num_devices, 0);
  for (int i = 0; i < num_devices; ++i) {
    g->rows[i] = (H - i + num_devices - 1) / num_devices;
    if (i >= 1) {
      g->recv_off[i] = g->recv_pixels;
      g->recv_pixels += (size_t)g->rows[i] * W;
    }
    PtOptions opt{};
    if (base) opt = *base;
    opt.device = devices[i];
    opt.pixel_begin = i * W;
    opt.pixel_count = g->rows[i] * W;
    opt.stripe_pixels = num_devices > 1 ? W : 0;
    opt.stripe_stride = num_devices > 1 ? num_devices * W : 0;
    PtContext* c = nullptr;
    if (pt_ctx_create(scene, &opt, &c)) {
      release(g);
      return -1;
    }
    g->ctx.push_back(c);
  }
  if (g->transport == PT_GROUP_TRANSPORT_COPY) {
    g->ready.assign(num_devices, nullptr);
    for (int i = 1; i < num_devices; ++i)
      if (hipSetDevice(devices[i]) != hipSuccess || hipEventCreateWithFlags(&g->ready[i], hipEventDisableTiming) != hipSuccess) {
        release(g);
        return pt_fail("pt_group_create: cannot create the tile-ready event on device %d", devices[i]);
      }
  } else {
    g->comms.assign(num_devices, nullptr);
    ncclResult_t r = ncclCommInitAll(g->comms.data(), num_devices, g->devices.data());
    if (r != ncclSuccess) {
      release(g);
      return pt_fail("ncclCommInitAll(%d devices) failed: %s", num_devices, ncclGetErrorString(r));
    }
  }
  *out = g;
  return 0;
}

int pt_group_create(const PtSceneDesc* scene, const PtOptions* base, const int* devices, int num_devices, PtGroup** out) {
  return pt_group_create_ex(scene, base, devices, num_devices, PT_GROUP_TRANSPORT_AUTO, out);
}

int pt_group_transport(const PtGroup* g) { return g ? g->transport : -1; }

int pt_group_destroy(PtGroup* g) {
  release(g);
  return 0;
}
int pt_group_size(const PtGroup* g) { return g ? g->n : 0; }
PtContext* pt_group_context(PtGroup* g, int i) { return (g && i >= 0 && i < g->n) ? g->ctx[i] : nullptr; }

int pt_group_render(PtGroup* g, int iter_first, int iter_count) {
  if (!g) return pt_fail("pt_group_render: null group");
  for (PtContext* c : g->ctx)  // launches are asynchronous: the devices run concurrently
    if (pt_ctx_render(c, iter_first, iter_count)) return -1;
  return 0;
}

int pt_group_sync(PtGroup* g) {
  if (!g) return pt_fail("pt_group_sync: null group");
  for (PtContext* c : g->ctx)
    if (pt_ctx_sync(c)) return -1;
  return 0;
}

int pt_group_gather(PtGroup* g, float* rgb_sum_host) {
  if (!g || !rgb_sum_host) return pt_fail("pt_group_gather: bad argument");
  const size_t frame = (size_t)g->W * g->H;
  HIP_OK(hipSetDevice(g->devices[0]));
  if (g->n == 1) return pt_ctx_readback(g->ctx[0], rgb_sum_host);
  if (assemble_image(g)) return -1;
  HIP_OK(hipMemcpyAsync(rgb_sum_host, g->d_full, frame * 12, hipMemcpyDeviceToHost, (hipStream_t)pt_ctx_stream(g->ctx[0])));
  return pt_group_sync(g);
}

// First-hit feature buffers (pt_ctx_render_features) of the whole frame: every context sums its own rows; the planes meet like
// the image, one exchange + row placement per plane with 16 bytes per pixel.
int pt_group_render_features(PtGroup* g, int iter_first, int iter_count) {
  if (!g) return pt_fail("pt_group_render_features: null group");
  for (PtContext* c : g->ctx)
    if (pt_ctx_render_features(c, iter_first, iter_count)) return -1;
  return 0;
}

int pt_group_gather_features(PtGroup* g, float* planes_host) {
  if (!g || !planes_host) return pt_fail("pt_group_gather_features: bad argument");
  const size_t frame = (size_t)g->W * g->H;
  if (need_features(g, "pt_group_gather_features")) return -1;
  HIP_OK(hipSetDevice(g->devices[0]));
  if (g->n == 1) return pt_ctx_readback_features(g->ctx[0], planes_host);
  if (assemble_features(g)) return -1;
  HIP_OK(hipMemcpyAsync(planes_host, g->d_full_feat, PT_FEATURE_PLANES * frame * 16, hipMemcpyDeviceToHost, (hipStream_t)pt_ctx_stream(g->ctx[0])));
  return pt_group_sync(g);
}

// pt_denoise of the whole frame: a context owns interleaved rows and cannot filter its own tile, so the SUM image and the planes
// meet on the root device as for the two gathers, and the launcher every context uses runs there on the root's stream.
int pt_group_denoise(PtGroup* g, float samples, const PtDenoiseOptions* opt, float* rgb_avg_host) {
  if (!g || !rgb_avg_host) return pt_fail("pt_group_denoise: bad argument");
  if (g->n == 1) return pt_ctx_denoise(g->ctx[0], samples, opt, rgb_avg_host);
  const size_t frame = (size_t)g->W * g->H;
  for (PtContext* c : g->ctx)  // (a group's rounds bring its contexts into the adaptive state: one sample count no longer describes the image)
    if (pt_ctx_admit_state(c, "pt_group_denoise", true)) return -1;
  if (need_features(g, "pt_group_denoise")) return -1;
  ptdn::Params P{};
  if (pt_denoise_resolve("pt_group_denoise", samples, opt, &P)) return -1;
  HIP_OK(hipSetDevice(g->devices[0]));
  if (!g->d_denoise) HIP_OK(hipMalloc(&g->d_denoise, pt_denoise_workspace_bytes(frame)));
  if (assemble_image(g) || assemble_features(g)) return -1;
  hipStream_t root = (hipStream_t)pt_ctx_stream(g->ctx[0]);
  const float* d_out = nullptr;
  if (pt_denoise_launch(root, g->W, g->H, g->d_full, g->d_full_feat, samples, P, g->d_denoise, &d_out)) return fail_after_drain(g);
  HIP_OK(hipMemcpyAsync(rgb_avg_host, d_out, frame * 12, hipMemcpyDeviceToHost, root));
  return pt_group_sync(g);
}

// pt_denoise_guided of the whole frame: as above, and the noise planes meet on the root like the feature planes.  The filter has ONE
// M and T, so the contexts must agree on them (and none may hold unfolded iterations: its own call would be refused).
int pt_group_denoise_guided(PtGroup* g, const PtDenoiseOptions* opt, float* rgb_avg_host) {
  if (!g || !rgb_avg_host) return pt_fail("pt_group_denoise_guided: bad argument");
  if (g->n == 1) return pt_ctx_denoise_guided(g->ctx[0], opt, rgb_avg_host);
  const size_t frame = (size_t)g->W * g->H;
  for (PtContext* c : g->ctx)
    if (pt_ctx_admit_state(c, "pt_group_denoise_guided", true)) return -1;
  if (need_features(g, "pt_group_denoise_guided")) return -1;
  int groups = 0, iters = 0;
  for (int i = 0; i < g->n; ++i) {
    int m = 0, t = 0;
    if (pt_ctx_get_noise(g->ctx[i], nullptr, &m, &t)) return -1;
    if (!pt_ctx_device_noise(g->ctx[i]) || m < 1) return pt_fail("pt_group_denoise_guided: nothing has been folded (pt_group_noise_fold)");
    if (pt_ctx_unfolded_iterations(g->ctx[i]) != 0) return pt_fail("pt_group_denoise_guided: context %d has iterations rendered since its last fold; fold first (pt_group_noise_fold)", i);
    if (i == 0) groups = m, iters = t;
    else if (m != groups || t != iters)
      return pt_fail("pt_group_denoise_guided: context %d folded %d groups of %d iterations, context 0 %d of %d; the contexts of a group share them", i, m, t, groups, iters);
  }
  ptdn::Params P{};
  float Tf = 0.0f, Df = 0.0f;
  if (pt_denoise_guided_resolve("pt_group_denoise_guided", groups, iters, opt, &P, &Tf, &Df)) return -1;
  HIP_OK(hipSetDevice(g->devices[0]));
  if (!g->d_denoise) HIP_OK(hipMalloc(&g->d_denoise, pt_denoise_workspace_bytes(frame)));
  if (assemble_image(g) || assemble_features(g) || assemble_noise(g)) return -1;
  hipStream_t root = (hipStream_t)pt_ctx_stream(g->ctx[0]);
  const float* d_out = nullptr;
  if (pt_denoise_guided_launch(root, g->W, g->H, g->d_full, g->d_full_feat, g->d_full_noise, Tf, Df, P, g->d_denoise, &d_out)) return fail_after_drain(g);
  HIP_OK(hipMemcpyAsync(rgb_avg_host, d_out, frame * 12, hipMemcpyDeviceToHost, root));
  return pt_group_sync(g);
}

// The noise estimate of the whole frame (pt_ctx_noise_fold): every context folds its own rows on its own stream, nothing is exchanged;
// the estimates meet on the host, one double per context.
int pt_group_noise_fold(PtGroup* g) {
  if (!g) return pt_fail("pt_group_noise_fold: null group");
  for (PtContext* c : g->ctx)
    if (pt_ctx_noise_fold(c)) return -1;
  return 0;
}

int pt_group_get_noise(PtGroup* g, double* sse, int* groups, int* iterations) {
  if (!g) return pt_fail("pt_group_get_noise: null group");
  double total = 0.0;
  for (int i = 0; i < g->n; ++i) {  // context order
    double part = -1.0;
    if (pt_ctx_get_noise(g->ctx[i], &part, i == 0 ? groups : nullptr, i == 0 ? iterations : nullptr)) return -1;
    total = (total < 0.0 || part < 0.0) ? -1.0 : total + part;
  }
  if (sse) *sse = total;
  return 0;
}

int pt_group_render_until(PtGroup* g, int iter_first, int max_iters, int group_iters, float target_db, int* iters_done, float* psnr_db) {
  if (!g) return pt_fail("pt_group_render_until: null group");
  if (iter_first < 1 || max_iters < 1 || (int64_t)iter_first + max_iters - 1 > INT32_MAX || group_iters < 0 || !std::isfinite(target_db))
    return pt_fail("pt_group_render_until: iterations %d, +%d in groups of %d until %g dB: the first is >= 1, the count >= 1, the group >= 0 (0 = a batch), the target finite",
                   iter_first, max_iters, group_iters, (double)target_db);
  int group = group_iters;
  if (!group) {
    PtStats st;
    if (pt_ctx_get_stats(g->ctx[0], &st)) return -1;
    group = st.iters_per_batch;
  }
  int done = 0;
  float psnr = -1.0f;
  while (done < max_iters) {
    const int n = group < max_iters - done ? group : max_iters - done;
    if (pt_group_render(g, iter_first + done, n)) return -1;
    done += n;
    double sse = -1.0;
    if (pt_group_noise_fold(g) || pt_group_get_noise(g, &sse, nullptr, nullptr)) return -1;
    if (sse < 0.0) continue;
    psnr = pt_psnr_from_sse(sse, (int64_t)g->W * g->H);
    if (psnr > target_db) break;
  }
  if (iters_done) *iters_done = done;
  if (psnr_db) *psnr_db = psnr;
  return 0;
}

// ---- adaptive sampling by threshold across the group: the frame's selection once, on the root; every context renders and merges its
// own part (group_round above).  Everything a single context would hold after the same calls, the contexts hold between them, bit for bit.
int pt_group_adaptive_round_threshold(PtGroup* g, int iter_first, int group_iters, float threshold, float max_fraction, int* above, int* selected) {
  if (!g) return pt_fail("pt_group_adaptive_round_threshold: null group");
  if (g->n == 1) return pt_ctx_adaptive_round_threshold(g->ctx[0], iter_first, group_iters, threshold, max_fraction, above, selected);
  return group_round(g, "pt_group_adaptive_round_threshold", iter_first, group_iters, threshold, max_fraction, 0, above, selected);
}

// pt_ctx_render_threshold's loop over pt_group_render, pt_group_noise_fold and the round above.
int pt_group_render_threshold(PtGroup* g, int iter_first, int max_iters, int group_iters, float threshold, float max_fraction, int min_pixels,
                              int* iters_done, int64_t* samples_done, int* above_left) {
  const char* who = "pt_group_render_threshold";
  if (!g) return pt_fail("%s: null group", who);
  if (g->n == 1)
    return pt_ctx_render_threshold(g->ctx[0], iter_first, max_iters, group_iters, threshold, max_fraction, min_pixels, iters_done, samples_done, above_left);
  if (max_iters < 1 || (int64_t)iter_first + max_iters - 1 > INT32_MAX || group_iters < 0 || min_pixels < 0)
    return pt_fail("%s: iterations %d, +%d in groups of %d until at most %d pixels are above: the count is >= 1, the group >= 0 (0 = a batch), the pixels >= 0", who,
                   iter_first, max_iters, group_iters, min_pixels);
  // what a round would refuse, apart from the state of the folds, which the uniform groups below establish
  for (PtContext* c : g->ctx)
    if (pt_ctx_adaptive_refusal(c, who, iter_first, group_iters, max_fraction, false)) return -1;
  if (pt_adaptive_check_threshold(who, threshold)) return -1;
  int group = group_iters;
  if (!group) {
    PtStats st;
    if (pt_ctx_get_stats(g->ctx[0], &st)) return -1;
    group = st.iters_per_batch;
  }
  int done = 0, above = -1;
  int64_t samples = 0;
  while (done < max_iters) {
    const int n = group < max_iters - done ? group : max_iters - done;
    PtCtxState s{};
    if (shared_state(g, who, &s)) return -1;
    if (!s.adaptive && s.groups < 2) {  // a uniform group and its fold
      if (pt_group_render(g, iter_first + done, n) || pt_group_noise_fold(g)) return -1;
      samples += (int64_t)n * g->W * g->H;
    } else {
      if (!s.adaptive && pt_group_noise_fold(g)) return -1;  // iterations of the caller's, not yet folded (a context without any folds nothing)
      int m = 0;
      if (group_round(g, who, iter_first + done, n, threshold, max_fraction, min_pixels, &above, &m)) return -1;
      if (above <= min_pixels) break;  // nothing was rendered
      samples += (int64_t)n * m;
    }
    done += n;
  }
  if (iters_done) *iters_done = done;
  if (samples_done) *samples_done = samples;
  if (above_left) *above_left = above;
  return 0;
}

// The per-pixel counts of the whole frame: in the adaptive state the count planes meet like a plane of 8 bytes per pixel; in the
// uniform state every pixel has the shared (T, M), as pt_readback_adaptive reports them.
int pt_group_gather_adaptive(PtGroup* g, int32_t* counts) {
  if (!g || !counts) return pt_fail("pt_group_gather_adaptive: bad argument");
  if (g->n == 1) return pt_ctx_readback_adaptive(g->ctx[0], counts);
  const size_t frame = (size_t)g->W * g->H;
  PtCtxState s{};
  if (shared_state(g, "pt_group_gather_adaptive", &s)) return -1;
  if (!s.adaptive) {
    if (pt_group_sync(g)) return -1;
    for (size_t p = 0; p < frame; ++p) counts[2 * p] = (int32_t)std::min<int64_t>(s.iters, INT32_MAX), counts[2 * p + 1] = s.groups;
    return 0;
  }
  std::vector<const int32_t*> tiles(g->n, nullptr);
  for (int i = 0; i < g->n; ++i) tiles[i] = pt_ctx_device_counts(g->ctx[i]);
  if (assemble_pairs(g, tiles)) return -1;
  HIP_OK(hipMemcpyAsync(counts, g->d_full_pair, frame * 8, hipMemcpyDeviceToHost, (hipStream_t)pt_ctx_stream(g->ctx[0])));
  return pt_group_sync(g);
}

// pt_resolve of the whole frame: every context resolves its own rows; the rows meet like the image (and in its buffers).
int pt_group_resolve(PtGroup* g, float* rgb_avg_host) {
  if (!g || !rgb_avg_host) return pt_fail("pt_group_resolve: bad argument");
  if (g->n == 1) return pt_ctx_resolve(g->ctx[0], rgb_avg_host);
  const size_t frame = (size_t)g->W * g->H;
  std::vector<const float*> tiles(g->n, nullptr);
  for (int i = 0; i < g->n; ++i)
    if (pt_ctx_resolve_device(g->ctx[i], &tiles[i])) return -1;
  HIP_OK(hipSetDevice(g->devices[0]));
  if (!g->d_full) HIP_OK(hipMalloc((void**)&g->d_full, frame * 12));
  if (!g->d_recv) HIP_OK(hipMalloc((void**)&g->d_recv, g->recv_pixels * 12));
  if (exchange(g, ncclFloat, 3, g->d_recv, [&](int i) { return tiles[i]; })) return fail_after_drain(g);
  HIP_OK(hipSetDevice(g->devices[0]));
  for (int i = 0; i < g->n; ++i)
    if (place_rows(g, i, i == 0 ? tiles[0] : g->d_recv + 3 * g->recv_off[i], g->d_full, 12)) return fail_after_drain(g);
  HIP_OK(hipMemcpyAsync(rgb_avg_host, g->d_full, frame * 12, hipMemcpyDeviceToHost, (hipStream_t)pt_ctx_stream(g->ctx[0])));
  return pt_group_sync(g);
}

// pt_denoise_adaptive of the whole frame: as pt_group_denoise_guided, and in the adaptive state the count planes meet on the root too
// (the uniform state: the launcher gives every pixel the shared (T, M), as it does for a context).  Refuses what the context's
// function refuses, in its order, each condition over the contexts in turn.
int pt_group_denoise_adaptive(PtGroup* g, const PtDenoiseOptions* opt, float* rgb_avg_host) {
  const char* who = "pt_group_denoise_adaptive";
  if (!g || !rgb_avg_host) return pt_fail("%s: bad argument", who);
  if (g->n == 1) return pt_ctx_denoise_adaptive(g->ctx[0], opt, rgb_avg_host);
  const size_t frame = (size_t)g->W * g->H;
  for (PtContext* c : g->ctx)
    if (pt_ctx_admit_state(c, who, false)) return -1;
  if (need_features(g, who)) return -1;
  for (PtContext* c : g->ctx)
    if (!pt_ctx_device_noise(c) || pt_ctx_state(c).groups < 1) return pt_fail("%s: nothing has been folded (pt_group_noise_fold)", who);
  for (int i = 0; i < g->n; ++i)
    if (pt_ctx_state(g->ctx[i]).unfolded != 0)
      return pt_fail("%s: context %d has iterations rendered since its last fold; fold first (pt_group_noise_fold)", who, i);
  PtCtxState s{};
  if (shared_state(g, who, &s)) return -1;
  if (s.groups < 2) return pt_fail("%s: %d group(s) folded; a variance needs at least 2 (pt_group_noise_fold after each group of iterations)", who, s.groups);
  if (s.iters > INT32_MAX) return pt_fail("%s: %lld iterations folded: the per-pixel counts are int32", who, (long long)s.iters);
  ptdn::Params P{};
  if (pt_denoise_adaptive_resolve(who, opt, &P)) return -1;
  HIP_OK(hipSetDevice(g->devices[0]));
  if (!g->d_denoise) HIP_OK(hipMalloc(&g->d_denoise, pt_denoise_workspace_bytes(frame)));
  if (assemble_image(g) || assemble_features(g) || assemble_noise(g)) return -1;
  if (s.adaptive) {
    std::vector<const int32_t*> tiles(g->n, nullptr);
    for (int i = 0; i < g->n; ++i) tiles[i] = pt_ctx_device_counts(g->ctx[i]);
    if (assemble_pairs(g, tiles)) return -1;
  }
  hipStream_t root = (hipStream_t)pt_ctx_stream(g->ctx[0]);
  const float* d_out = nullptr;
  if (pt_denoise_adaptive_launch(root, g->W, g->H, g->d_full, g->d_full_feat, g->d_full_noise, s.adaptive ? g->d_full_pair : nullptr, (int)s.iters, s.groups, P,
                                 g->d_denoise, &d_out))
    return fail_after_drain(g);
  HIP_OK(hipMemcpyAsync(rgb_avg_host, d_out, frame * 12, hipMemcpyDeviceToHost, root));
  return pt_group_sync(g);
}

int pt_group_gather_u8(PtGroup* g, float samples, uint8_t* rgb8_host) {
  if (!g || !rgb8_host) return pt_fail("pt_group_gather_u8: bad argument");
  const size_t frame = (size_t)g->W * g->H;
  std::vector<const uint8_t*> tiles(g->n, nullptr);
  for (int i = 0; i < g->n; ++i)  // every device converts its own rows (x mirror is inside a row)
    if (pt_ctx_save_u8_device(g->ctx[i], samples, &tiles[i])) return -1;
  HIP_OK(hipSetDevice(g->devices[0]));
  if (g->n == 1) {
    HIP_OK(hipMemcpyAsync(rgb8_host, tiles[0], frame * 3, hipMemcpyDeviceToHost, (hipStream_t)pt_ctx_stream(g->ctx[0])));
    return pt_group_sync(g);
  }
  if (!g->d_full8) HIP_OK(hipMalloc((void**)&g->d_full8, frame * 3));
  if (!g->d_recv8) HIP_OK(hipMalloc((void**)&g->d_recv8, g->recv_pixels * 3));
  if (exchange(g, ncclUint8, 3, g->d_recv8, [&](int i) { return tiles[i]; })) return fail_after_drain(g);
  HIP_OK(hipSetDevice(g->devices[0]));
  for (int i = 0; i < g->n; ++i)
    if (place_rows(g, i, i == 0 ? tiles[0] : g->d_recv8 + 3 * g->recv_off[i], g->d_full8, 3)) return fail_after_drain(g);
  HIP_OK(hipMemcpyAsync(rgb8_host, g->d_full8, frame * 3, hipMemcpyDeviceToHost, (hipStream_t)pt_ctx_stream(g->ctx[0])));
  return pt_group_sync(g);
}

// Convergence metric of the whole frame (PtOptions.convergence in `base`): every context keeps the sums of its own rows; they
// meet on the host, one double per iteration and context.
int pt_group_set_reference(PtGroup* g, const float* rgb_avg_host) {
  if (!g || !rgb_avg_host) return pt_fail("pt_group_set_reference: bad argument");
  const size_t row = 3 * (size_t)g->W;
  std::vector<float> tile;
  for (int i = 0; i < g->n; ++i) {  // context i owns rows i, i + n, ... in that order
    tile.resize(row * (size_t)g->rows[i]);
    for (int r = 0; r < g->rows[i]; ++r) std::memcpy(tile.data() + row * r, rgb_avg_host + row * ((size_t)i + (size_t)r * g->n), row * sizeof(float));
    if (pt_ctx_set_reference(g->ctx[i], tile.data())) return -1;
  }
  return 0;
}

int pt_group_get_convergence(PtGroup* g, int iter_first, int iter_count, double* sse) {
  if (!g || iter_count < 0 || (iter_count > 0 && !sse)) return pt_fail("pt_group_get_convergence: bad argument");
  std::vector<double> part((size_t)iter_count);
  for (int i = 0; i < g->n; ++i) {
    if (pt_ctx_get_convergence(g->ctx[i], iter_first, iter_count, i == 0 ? sse : part.data())) return -1;
    for (int j = 0; j < iter_count && i > 0; ++j) sse[j] = (sse[j] < 0.0 || part[j] < 0.0) ? -1.0 : sse[j] + part[j];  // context order
  }
  return 0;
}

int pt_group_iterations_to_clean(PtGroup* g, float threshold_db, int* iteration) {
  if (!g || !iteration) return pt_fail("pt_group_iterations_to_clean: bad argument");
  *iteration = -1;
  const int chunk = 1024;
  std::vector<double> sse((size_t)chunk);
  for (int first = 1; first <= PT_CONVERGENCE_CAPACITY; first += chunk) {
    if (pt_group_get_convergence(g, first, chunk, sse.data())) return -1;
    bool any = false;
    for (int j = 0; j < chunk; ++j) {
      if (sse[j] < 0.0) continue;
      any = true;
      if (pt_psnr_from_sse(sse[j], (int64_t)g->W * g->H) > threshold_db) {
        *iteration = first + j;
        return 0;
      }
    }
    if (!any && first > 1) break;  // past the rendered iterations
  }
  return 0;
}

// Progressive preview (the reference converts and shows the running average after EVERY iteration: sendImageToPBO,
// src/pathtrace.cu:250-268,618): every device converts its own rows (average over `iterations`, gamma 1/2.2, clamp,
// RGBA8), then the same single exchange + row placement as the write-out, 4 B per pixel.  Meant to be called every N
// batches while rendering continues; it synchronises the devices (the image is read at a batch boundary).
int pt_group_preview_rgba8(PtGroup* g, int iterations, uint8_t* rgba_host) {
  if (!g || !rgba_host || iterations <= 0) return pt_fail("pt_group_preview_rgba8: bad argument");
  const size_t frame = (size_t)g->W * g->H;
  if (g->d_prev.empty()) g->d_prev.assign(g->n, nullptr);
  for (int i = 0; i < g->n; ++i) {
    HIP_OK(hipSetDevice(g->devices[i]));
    if (!g->d_prev[i]) HIP_OK(hipMalloc((void**)&g->d_prev[i], (size_t)pt_ctx_pixel_count(g->ctx[i]) * 4));
    if (pt_ctx_preview_rgba8_device(g->ctx[i], iterations, g->d_prev[i])) return -1;
  }
  HIP_OK(hipSetDevice(g->devices[0]));
  if (g->n == 1) {
    HIP_OK(hipMemcpyAsync(rgba_host, g->d_prev[0], frame * 4, hipMemcpyDeviceToHost, (hipStream_t)pt_ctx_stream(g->ctx[0])));
    return pt_group_sync(g);
  }
  if (!g->d_full_prev) HIP_OK(hipMalloc((void**)&g->d_full_prev, frame * 4));  // kept in the group: previews recur every
  if (!g->d_recv_prev) HIP_OK(hipMalloc((void**)&g->d_recv_prev, g->recv_pixels * 4));  // few batches; freed by release()
  if (exchange(g, ncclUint8, 4, g->d_recv_prev, [&](int i) { return (const uint8_t*)g->d_prev[i]; })) return fail_after_drain(g);
  HIP_OK(hipSetDevice(g->devices[0]));
  for (int i = 0; i < g->n; ++i)
    if (place_rows(g, i, i == 0 ? (const uint8_t*)g->d_prev[0] : g->d_recv_prev + 4 * g->recv_off[i], g->d_full_prev, 4))
      return fail_after_drain(g);
  HIP_OK(hipMemcpyAsync(rgba_host, g->d_full_prev, frame * 4, hipMemcpyDeviceToHost, (hipStream_t)pt_ctx_stream(g->ctx[0])));
  return pt_group_sync(g);
}

}  // extern "C"
