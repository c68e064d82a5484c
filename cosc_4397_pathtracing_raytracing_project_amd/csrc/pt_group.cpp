// pt_group.cpp — one process, several MI355X: BASELINE config 4 (framebuffer tiled across the GPUs of a node, a
// single RCCL gather over xGMI at image write-out; SURVEY.md §8e, §5 "Distributed communication backend").
//
// The reference is single-device (src/preview.cpp:112 cudaGLSetGLDevice(0)); its write-out point is saveImage()
// (src/main.cpp:86-107).  Here every device owns the rows i, i+n, i+2n, ... of the frame (work per row varies
// smoothly down the cornell frame, interleaving gives every device the same mix) and runs ALL iterations on them
// on its own stream; samples are keyed by the global pixel index (makeSeededRandomEngine(iter, idx, depth),
// src/pathtrace.cu:203-207,368), so nothing is ever summed across devices and the assembled image is bit-identical
// to the single-GPU image.  The only communication towards the root is, once per write-out, one grouped ncclSend/ncclRecv
// of the tiles into devices[0] on a ncclCommInitAll communicator — xGMI is point-to-point, the tiles go straight to the
// root over their own links, there is no ring and no reduction.  Placement of the interleaved rows (a strided 2-D
// copy on the root device) and one D2H copy follow.
//
// Every write-out is that one path, gather(), with a payload of B bytes per pixel (Payload below): the SUM image and the resolved
// image (12 B), a feature or noise plane (16 B, one exchange per plane), the packed {w, T} pairs of a round and the count planes (8 B),
// the converted bytes (3 B) and the preview (4 B).  The tiles meet in ONE receive buffer of 16 B per received pixel (PtGroup::d_recv);
// each payload has a frame buffer of its own, since a filter reads several of them in one launch.  The one exchange in the other
// direction, the parts of the frame's list back to the contexts, is scatter_parts().
//
// Two transports for those exchanges (PtGroup::transport, pt_group_create_ex):
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
#include <utility>
#include <vector>

#include "pt_adaptive.h"
#include "pt_context.h"  // HIP_OK; a group reaches its contexts through the C ABI and the helpers declared there
#include "pt_denoise.h"
#include "pt_group_select.h"
#include "pt_history.h"
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
  std::vector<std::pair<int, void*>> owned;  // (device, buffer): every device buffer below; ensure() allocates it at its first use, release() frees it
  int64_t owned_bytes = 0;                   // what `owned` adds up to (pt_group_device_bytes)
  // root: THE receive buffer of every write-out, the tiles of devices 1..n-1 back to back, kRecvBytes (the widest payload) per pixel.
  // Payloads of different widths follow each other in it with nothing but stream order between them.  That is sound because all three
  // parties are queued on the ROOT context's stream: the COPY transport's copies into it, RCCL's ncclRecv into it, and the placement
  // of the rows that reads it.  A plane that follows a plane (gather_planes) is a case of it.
  char* d_recv = nullptr;
  // root: the assembled frames, one per payload — a filter reads the image, the planes and the pairs in one launch
  float* d_full = nullptr;          // the SUM image; the resolved image
  uint8_t* d_full8 = nullptr;       // the converted bytes (3 B/pixel)
  uint8_t* d_full_prev = nullptr;   // the RGBA8 preview (kept: previews recur)
  float* d_full_feat = nullptr;     // the feature planes
  float* d_full_noise = nullptr;    // the noise planes (pt_group_denoise_guided)
  int32_t* d_full_pair = nullptr;   // 8 B per pixel: the packed pairs of a round; the count planes at write-out
  void* d_denoise = nullptr;        // root: workspace of pt_group_denoise over the whole frame
  std::vector<uint8_t*> d_prev;     // per device: RGBA8 preview of its tile (sendImageToPBO)
  // Adaptive sampling by threshold (pt_group_adaptive_round_threshold); all of it absent until the first round
  std::vector<void*> d_pack;       // per context, on its device: {w_p, T_p} of its tile, 8 B per pixel
  std::vector<int32_t*> d_part;    // per context i >= 1, on its device: its part of the frame's list
  void* d_select = nullptr;        // root: the selection's workspace for W*H pixels (pt_adaptive_select_bytes)
  void* d_partition = nullptr;     // root: the partition's workspace (pt_group_partition_bytes)
  int32_t* d_list = nullptr;       // root: the frame's list, W*H entries, the first m in use
  int32_t* d_parts = nullptr;      // root: the contexts' lists back to back
  uint32_t* d_result = nullptr;    // root: above, m, m_0 .. m_(n-1)
  hipEvent_t parts_ready = nullptr;  // root: the parts are complete (recorded on the root's stream)
  // The reprojected history of the frame (pt_group_history_*): the single context's state (pt_context.h) over W*H pixels, all of it on
  // the root and absent until the first capture.  pt_group_clear, pt_group_set_camera[_ex] and pt_group_set_geoms make C and VC absent.
  void* d_hist = nullptr;            // root: pt_history_state_bytes(W*H): the kept planes K0 K1 K2, then the current plane C
  void* d_hist_var = nullptr;        // root: pt_history_variance_bytes(W*H): VK, then VC; from the first capture with PT_HISTORY_MOMENTS
  float* d_blend = nullptr;          // root: the blend of pt_group_history_resolve, W*H*3 floats
  float* d_full_extra = nullptr;     // root: the assembled extra plane E, W*H floats
  hipEvent_t tiles_read = nullptr;   // root, COPY transport: the root's stream has read the tiles (release_tiles)
  PtCamera hist_cam{};               // the camera K is aligned to
  bool hist_kept = false;            // K holds a capture (pt_group_history_drop forgets it)
  bool hist_current = false;         // C holds a lookup for the current camera
  uint32_t hist_var_kept = 0;        // the kind VK holds: 0 (a plain capture) or PT_HISTORY_MOMENTS
  uint32_t hist_var_current = 0;     // ... and VC; 0 whenever C is absent
  PtHistoryMotion hist_motion;       // the kept geoms with their stale flag and the motion table (its device copy: context 0's)
};

namespace {

// What one pixel of a write-out is: `bytes` to the copies and the placement, `elems` elements of `type` to RCCL.
struct Payload {
  size_t bytes;
  ncclDataType_t type;
  int elems;
};
constexpr size_t kRecvBytes = 16;  // per pixel of PtGroup::d_recv
constexpr Payload kRgb{12, ncclFloat, 3}, kPlane{16, ncclFloat, 4}, kPair{8, ncclInt32, 2}, kRgb8{3, ncclUint8, 3}, kRgba8{4, ncclUint8, 4}, kExtra{4, ncclFloat, 1};
constexpr bool payload_ok(Payload p, size_t elem_bytes) { return p.bytes == p.elems * elem_bytes && p.bytes <= kRecvBytes; }
static_assert(payload_ok(kRgb, 4) && payload_ok(kPlane, 4) && payload_ok(kPair, 4) && payload_ok(kRgb8, 1) && payload_ok(kRgba8, 1) && payload_ok(kExtra, 4), "a payload wider than the receive buffer's pixel");

size_t frame_pixels(const PtGroup* g) { return (size_t)g->W * g->H; }
hipStream_t stream(const PtGroup* g, int i) { return (hipStream_t)pt_ctx_stream(g->ctx[i]); }

// A buffer of the group's that exists from its first use on (a context's is ptc::ensure): `bytes` on devices[i], which is current.
template <typename T>
int ensure(PtGroup* g, int i, T*& p, size_t bytes) {
  if (p) return 0;
  HIP_OK(hipMalloc((void**)&p, bytes));
  g->owned.emplace_back(g->devices[i], p);
  g->owned_bytes += (int64_t)bytes;
  return 0;
}

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
  if (g->parts_ready) (void)hipEventDestroy(g->parts_ready);
  if (g->tiles_read) (void)hipEventDestroy(g->tiles_read);
  for (const auto& [device, p] : g->owned) {
    (void)hipSetDevice(device);
    (void)hipFree(p);
  }
  for (PtContext* c : g->ctx) (void)pt_ctx_destroy(c);
  delete g;
}

// ---- the transport layer, both directions
// One RCCL group around `body`: an error inside the group must still close it, and the first error wins.
template <typename Body>
int rccl_group(Body body) {
  NCCL_OK(ncclGroupStart());
  int rc = body();
  const ncclResult_t e = ncclGroupEnd();
  if (!rc && e != ncclSuccess) rc = pt_fail("ncclGroupEnd failed: %s", ncclGetErrorString(e));
  return rc;
}

// COPY transport: `bytes` from context `from`'s device to context `to`'s, on `s`.
int copy_between(PtGroup* g, void* dst, int to, const void* src, int from, size_t bytes, hipStream_t s) {
  if (g->devices[to] == g->devices[from]) HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
  else HIP_OK(hipMemcpyPeerAsync(dst, g->devices[to], src, g->devices[from], bytes, s));
  return 0;
}

// The one exchange of a write-out: device i >= 1 hands the payload of its pixels at tile(i) to the root, which receives them back to
// back (recv_off) in d_recv on its stream.  RCCL: one grouped send/recv, each send on its own device's stream.  COPY: the root's
// stream waits for tile i's producer, then pulls the tile.
template <typename TileFn>
int exchange(PtGroup* g, Payload pl, TileFn tile) {
  hipStream_t root = stream(g, 0);
  if (g->transport == PT_GROUP_TRANSPORT_COPY) {
    for (int i = 1; i < g->n; ++i) {
      HIP_OK(hipSetDevice(g->devices[i]));
      HIP_OK(hipEventRecord(g->ready[i], stream(g, i)));
      HIP_OK(hipSetDevice(g->devices[0]));
      HIP_OK(hipStreamWaitEvent(root, g->ready[i], 0));
      if (copy_between(g, g->d_recv + pl.bytes * g->recv_off[i], 0, tile(i), i, pl.bytes * (size_t)pt_ctx_pixel_count(g->ctx[i]), root)) return -1;
    }
    return 0;
  }
  return rccl_group([&] {
    int rc = 0;
    for (int i = 1; i < g->n && !rc; ++i) {
      const size_t count = (size_t)pl.elems * pt_ctx_pixel_count(g->ctx[i]);
      ncclResult_t r = ncclSuccess;
      if (hipSetDevice(g->devices[i]) != hipSuccess) rc = pt_fail("hipSetDevice(%d) failed", g->devices[i]);
      else if ((r = ncclSend(tile(i), count, pl.type, 0, g->comms[i], stream(g, i))) != ncclSuccess)
        rc = pt_fail("ncclSend from device %d failed: %s", g->devices[i], ncclGetErrorString(r));
      else if (hipSetDevice(g->devices[0]) != hipSuccess) rc = pt_fail("hipSetDevice(%d) failed", g->devices[0]);
      else if ((r = ncclRecv(g->d_recv + pl.bytes * g->recv_off[i], count, pl.type, i, g->comms[0], root)) != ncclSuccess)
        rc = pt_fail("ncclRecv from device %d failed: %s", g->devices[i], ncclGetErrorString(r));
    }
    return rc;
  });
}

// After a failed exchange / placement some sends, receives or copies may already be queued on the devices' streams:
// drain them (ignoring further errors, keeping the first message) before the caller sees the failure.
int fail_after_drain(PtGroup* g) {
  const std::string first = pt_last_error();
  for (PtContext* c : g->ctx) (void)pt_ctx_sync(c);
  return pt_fail("%s", first.c_str());
}

// The way back, beside the root's own part at the head of d_parts: part i >= 1, counts[i] entries behind those of the contexts before
// it, to context i's d_part[i] on context i's stream; a part without entries is not sent.
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
int scatter_parts(PtGroup* g, const uint32_t* counts) {
  hipStream_t root = stream(g, 0);
  HIP_OK(hipEventRecord(g->parts_ready, root));
  std::vector<size_t> off(g->n, 0);
  for (int i = 1; i < g->n; ++i) off[i] = off[i - 1] + counts[i - 1];
  if (g->transport == PT_GROUP_TRANSPORT_COPY) {
    for (int i = 1; i < g->n; ++i) {
      HIP_OK(hipSetDevice(g->devices[i]));
      HIP_OK(hipStreamWaitEvent(stream(g, i), g->parts_ready, 0));
      if (counts[i] && copy_between(g, g->d_part[i], i, g->d_parts + off[i], 0, counts[i] * sizeof(int32_t), stream(g, i))) return -1;
    }
    return 0;
  }
  const int rc = rccl_group([&] {
    int rc = 0;
    for (int i = 1; i < g->n && !rc; ++i) {
      const size_t count = counts[i];
      if (!count) continue;
      ncclResult_t r = ncclSuccess;
      if (hipSetDevice(g->devices[0]) != hipSuccess) rc = pt_fail("hipSetDevice(%d) failed", g->devices[0]);
      else if ((r = ncclSend(g->d_parts + off[i], count, ncclInt32, i, g->comms[0], root)) != ncclSuccess)
        rc = pt_fail("ncclSend to device %d failed: %s", g->devices[i], ncclGetErrorString(r));
      else if (hipSetDevice(g->devices[i]) != hipSuccess) rc = pt_fail("hipSetDevice(%d) failed", g->devices[i]);
      else if ((r = ncclRecv(g->d_part[i], count, ncclInt32, 0, g->comms[i], stream(g, i))) != ncclSuccess)
        rc = pt_fail("ncclRecv on device %d failed: %s", g->devices[i], ncclGetErrorString(r));
    }
    return rc;
  });
  return rc ? fail_after_drain(g) : 0;
}

// ---- the write-outs
// The device side of every write-out (n > 1; the root device is current), on the root's stream: the payload of every context's tile
// (tile(i), on device i) through the receive buffer into plane `plane` of the `planes` frames of that payload in `full` — the exchange,
// then the rows of context i (tile order) to the rows i, i + n, ... of the frame.  What follows — a copy to the host, the selection, a
// filter — is queued behind them on the same stream.
template <typename T, typename TileFn>
int gather(PtGroup* g, Payload pl, TileFn tile, T*& full, int planes = 1, int plane = 0) {
  const size_t row = (size_t)g->W * pl.bytes;
  if (ensure(g, 0, full, planes * g->H * row) || ensure(g, 0, g->d_recv, g->recv_pixels * kRecvBytes)) return -1;
  if (exchange(g, pl, tile)) return fail_after_drain(g);
  char* frame = reinterpret_cast<char*>(full) + plane * g->H * row;
  hipError_t e = hipSetDevice(g->devices[0]);
  for (int i = 0; i < g->n && e == hipSuccess; ++i)
    e = hipMemcpy2DAsync(frame + i * row, g->n * row, i == 0 ? (const void*)tile(0) : g->d_recv + pl.bytes * g->recv_off[i], row, row, (size_t)g->rows[i],
                         hipMemcpyDeviceToDevice, stream(g, 0));
  if (e == hipSuccess) return 0;
  pt_fail("placing the rows of a %zu-byte payload failed: %s", pl.bytes, hipGetErrorString(e));
  return fail_after_drain(g);
}
// The tail of a write-out: `bytes` of a root buffer to the host on the root's stream, and every context synchronised.
int to_host(PtGroup* g, void* host, const void* d_root, size_t bytes) {
  HIP_OK(hipMemcpyAsync(host, d_root, bytes, hipMemcpyDeviceToHost, stream(g, 0)));
  return pt_group_sync(g);
}

int gather_image(PtGroup* g) {  // -> g->d_full: W*H*3 floats
  return gather(g, kRgb, [&](int i) { return pt_ctx_device_image(g->ctx[i]); }, g->d_full);
}
// `count` float4 planes of every context (planes(c): plane 0 of context c, the planes contiguous) -> full: the planes of the frame.
// One exchange and placement per plane: a tile's planes are its pixel_count apart, not recv_pixels.
template <typename PlanesFn>
int gather_planes(PtGroup* g, int count, float*& full, PlanesFn planes) {
  for (int pl = 0; pl < count; ++pl)
    if (gather(g, kPlane, [&](int i) { return planes(g->ctx[i]) + 4 * (size_t)pl * pt_ctx_pixel_count(g->ctx[i]); }, full, count, pl)) return -1;
  return 0;
}
int gather_features(PtGroup* g) {  // -> g->d_full_feat: PT_FEATURE_PLANES planes of W*H float4
  return gather_planes(g, PT_FEATURE_PLANES, g->d_full_feat, [](PtContext* c) { return pt_ctx_device_features(c); });
}
int gather_noise(PtGroup* g) {  // -> g->d_full_noise: PT_NOISE_PLANES planes of W*H float4
  return gather_planes(g, PT_NOISE_PLANES, g->d_full_noise, [](PtContext* c) { return pt_ctx_device_noise(c); });
}
int gather_counts(PtGroup* g) {  // -> g->d_full_pair: the count planes, 8 bytes per pixel (where a round has the packed pairs)
  return gather(g, kPair, [&](int i) { return pt_ctx_device_counts(g->ctx[i]); }, g->d_full_pair);
}

int need_features(PtGroup* g, const char* who) {
  for (PtContext* c : g->ctx)
    if (!pt_ctx_device_features(c)) return pt_fail("%s: no feature pass has been rendered (pt_group_render_features)", who);
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

// ---- the three filters of a group (n > 1), around what differs between them: the refusals in between and the launcher.
// The head, after the arguments: no context failed half-way (uniform: or is in the adaptive state), every context has its features.
int filter_admit(PtGroup* g, const char* who, bool uniform) {
  for (PtContext* c : g->ctx)  // (a group's rounds bring its contexts into the adaptive state: one sample count no longer describes the image)
    if (pt_ctx_admit_state(c, who, uniform) || pt_ctx_admit_no_extras(c, who)) return -1;  // (... nor do the extras of a history round)
  return need_features(g, who);
}
// The tail, after the last refusal: a context owns interleaved rows and cannot filter its own tile, so the SUM image, the feature
// planes and, where the filter reads them, the noise planes and the count planes meet on the root device as for the gathers, and the
// launcher every context uses (launch(stream, &d_out)) runs there on the root's stream over the whole frame.
template <typename Launch>
int filter_run(PtGroup* g, bool noise, bool counts, float* rgb_avg_host, Launch launch) {
  const size_t frame = frame_pixels(g);
  HIP_OK(hipSetDevice(g->devices[0]));
  if (ensure(g, 0, g->d_denoise, pt_denoise_workspace_bytes(frame))) return -1;
  if (gather_image(g) || gather_features(g) || (noise && gather_noise(g)) || (counts && gather_counts(g))) return -1;
  const float* d_out = nullptr;
  if (launch(stream(g, 0), &d_out)) return fail_after_drain(g);
  return to_host(g, rgb_avg_host, d_out, frame * 12);
}

// ---- what the group's two rounds (the threshold round, the history round) share around their keys
// The buffers of the frame's selection on the root and of the parts' way back, at the first round of either kind.
int selection_buffers(PtGroup* g) {
  const int n = g->n;
  const size_t frame = frame_pixels(g);
  HIP_OK(hipSetDevice(g->devices[0]));
  if (ensure(g, 0, g->d_select, pt_adaptive_select_bytes(frame)) || ensure(g, 0, g->d_partition, pt_group_partition_bytes(frame, n)) ||
      ensure(g, 0, g->d_list, frame * sizeof(int32_t)) || ensure(g, 0, g->d_parts, frame * sizeof(int32_t)) ||
      ensure(g, 0, g->d_result, (2 + (size_t)n) * sizeof(uint32_t)))
    return -1;
  if (!g->parts_ready) HIP_OK(hipEventCreateWithFlags(&g->parts_ready, hipEventDisableTiming));
  if (g->d_pack.empty()) g->d_pack.assign(n, nullptr), g->d_part.assign(n, nullptr);
  for (int i = 1; i < n; ++i) {
    HIP_OK(hipSetDevice(g->devices[i]));
    if (ensure(g, i, g->d_part[i], (size_t)pt_ctx_pixel_count(g->ctx[i]) * sizeof(int32_t))) return -1;
  }
  HIP_OK(hipSetDevice(g->devices[0]));
  return 0;
}
// d_result after the partition: {count, m, m_0 .. m_(n-1)}, 8 + 4n bytes behind ONE synchronise of the root's stream, and checked: the
// list fits the cap and the count (`count_name` in the message), the parts add up to it, every part fits its context.
int read_selection(PtGroup* g, const char* who, int cap, const char* count_name, std::vector<uint32_t>* out) {
  const int n = g->n;
  hipStream_t root = stream(g, 0);
  std::vector<uint32_t>& result = *out;
  result.assign(2 + (size_t)n, 0u);
  HIP_OK(hipMemcpyAsync(result.data(), g->d_result, result.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, root));
  HIP_OK(hipStreamSynchronize(root));
  const int m = (int)result[1];
  int64_t sum = 0;
  for (int i = 0; i < n; ++i) sum += result[2 + (size_t)i];
  bool fits = m >= 0 && m <= cap && (int)result[0] >= m && sum == m;
  for (int i = 0; i < n && fits; ++i) fits = (int64_t)result[2 + (size_t)i] <= pt_ctx_pixel_count(g->ctx[i]);
  if (!fits) return pt_fail("%s: the selection left %u %s, a list of %u (cap %d) in parts that add up to %lld", who, result[0], count_name, result[1], cap, (long long)sum);
  return 0;
}
int round_limits(PtGroup* g, const char* who) {
  if (g->n > ptgs::kMaxParts || g->H >= 32768 || frame_pixels(g) > ((size_t)1 << 30))
    return pt_fail("%s: %d contexts on a frame of %d x %d: at most %d contexts, fewer than 32768 rows, at most 2^30 pixels", who, g->n, g->W, g->H, ptgs::kMaxParts);
  return 0;
}

// One round of pt_group_adaptive_round_threshold for n > 1, after the arguments' refusals; the driver's min_pixels as in the context's round.
int group_round(PtGroup* g, const char* who, int iter_first, int group_iters, float threshold, float max_fraction, int min_pixels, int* above, int* selected) {
  const int n = g->n, W = g->W, H = g->H;
  const size_t frame = frame_pixels(g);
  for (int i = 0; i < n; ++i)
    if (pt_ctx_adaptive_refusal(g->ctx[i], who, iter_first, group_iters, max_fraction, true)) return -1;
  if (pt_adaptive_check_threshold(who, threshold)) return -1;
  if (round_limits(g, who)) return -1;
  PtCtxState shared{};
  if (shared_state(g, who, &shared)) return -1;
  const int cap = ptad::list_length((double)max_fraction, (int64_t)frame);
  hipStream_t root = stream(g, 0);

  // the group's buffers: the first round
  if (selection_buffers(g)) return -1;
  for (int i = 0; i < n; ++i) {
    HIP_OK(hipSetDevice(g->devices[i]));
    if (ensure(g, i, g->d_pack[i], (size_t)pt_ctx_pixel_count(g->ctx[i]) * 8)) return -1;
  }

  // collect on the root: every context packs on its own stream, one exchange, the rows into the frame, key, select, partition
  for (int i = 0; i < n; ++i) {
    if (pt_ctx_enter_adaptive(g->ctx[i])) return -1;
    HIP_OK(hipSetDevice(g->devices[i]));
    if (pt_group_pack_launch(stream(g, i), pt_ctx_pixel_count(g->ctx[i]), pt_ctx_device_noise(g->ctx[i]), pt_ctx_device_counts(g->ctx[i]), g->d_pack[i])) return -1;
  }
  HIP_OK(hipSetDevice(g->devices[0]));
  if (gather(g, kPair, [&](int i) { return g->d_pack[i]; }, g->d_full_pair)) return -1;
  if (pt_group_keys_launch(root, W, H, g->d_full_pair, pt_adaptive_select_keys(g->d_select, frame)) ||
      pt_adaptive_select_threshold_keys_launch(root, W, H, threshold, cap, g->d_select, g->d_list) ||
      pt_group_partition_launch(root, W, n, g->d_list, pt_adaptive_select_result(g->d_select, frame), cap, g->d_partition, g->d_parts, g->d_result))
    return fail_after_drain(g);

  // read back: above, m and the parts' lengths, 8 + 4n bytes and ONE synchronise
  std::vector<uint32_t> result;
  if (read_selection(g, who, cap, "above", &result)) return -1;
  const int m = (int)result[1];
  const bool render = m > 0 && (int)result[0] > min_pixels;
  if (above) *above = (int)result[0];
  if (selected) *selected = render ? m : 0;
  if (!render) return 0;  // nothing rendered or merged, no context counts a round

  // distribute and render: part i to context i, on context i's stream
  if (scatter_parts(g, result.data() + 2)) return -1;
  for (int i = 0; i < n; ++i) {  // asynchronous: the contexts render concurrently; a context without pixels counts the round
    const int pixels = pt_ctx_pixel_count(g->ctx[i]);
    if (pt_ctx_adaptive_round_list_device(g->ctx[i], iter_first, group_iters, i == 0 ? g->d_parts : g->d_part[i], (int)result[2 + (size_t)i], cap < pixels ? cap : pixels))
      return fail_after_drain(g);
  }
  return 0;
}

// group_iters == 0 means the iterations per batch of context 0 (pt_group_render_until, pt_group_render_threshold)
int group_or_batch(PtGroup* g, int group_iters, int* group) {
  PtStats st{};
  if (!group_iters && pt_ctx_get_stats(g->ctx[0], &st)) return -1;
  *group = group_iters ? group_iters : st.iters_per_batch;
  return 0;
}

// ---- the reprojected history of the frame (n > 1).  A context owns interleaved rows and cannot look up its neighbours, so every call
// follows the filters' shape: its refusals, the gathers of what it reads onto the root, the single context's launch on the root's
// stream over W*H pixels (the view: pthi::make_view(kept camera, H, 0)), to_host() where something is returned.  Nothing assembled is
// kept from one call to the next.
pthi::V4* history_plane(const PtGroup* g, int plane) { return static_cast<pthi::V4*>(g->d_hist) + (size_t)plane * frame_pixels(g); }  // K0 K1 K2, C
pthi::V4* history_var_plane(const PtGroup* g, int plane) { return static_cast<pthi::V4*>(g->d_hist_var) + (size_t)plane * frame_pixels(g); }  // 0: VK, 1: VC
const pthi::V4* current_plane(const PtGroup* g) { return g->hist_current ? history_plane(g, pthi::kKeptPlanes) : nullptr; }

// What pt_history_* refuses of any context, in the single context's order and apart from the tile's rows: a failed context, the flag
// word (check_flags()), the adaptive state, (features) no feature pass since the last clear or move.  Each condition over the contexts in turn.
template <typename Flags>
int history_admit(PtGroup* g, const char* who, bool features, Flags check_flags) {
  for (PtContext* c : g->ctx)
    if (pt_ctx_admit_state(c, who, false)) return -1;
  if (check_flags()) return -1;
  for (PtContext* c : g->ctx)
    if (pt_ctx_admit_state(c, who, true)) return -1;
  for (PtContext* c : g->ctx)
    if (features && !pt_ctx_features_fresh(c))
      return pt_fail("%s: no feature pass has been rendered since the last pt_group_clear or move (pt_group_render_features)", who);
  return 0;
}
int no_flags() { return 0; }
// The kinds and forms a group does not have, by name.
int history_not_built(const char* who, uint32_t flags) {
  if (flags & PT_HISTORY_VARIANCE) return pt_fail("%s: PT_HISTORY_VARIANCE is not built for a group (the moments kind is: PT_HISTORY_MOMENTS)", who);
  if (flags & PT_HISTORY_FEEDBACK) return pt_fail("%s: PT_HISTORY_FEEDBACK is not built for a group", who);
  if (flags & PT_HISTORY_MATERIALS) return pt_fail("%s: PT_HISTORY_MATERIALS is not built for a group", who);
  return 0;
}
int history_current_moments(const PtGroup* g, const char* who) {
  if (g->hist_current && g->hist_var_current != PT_HISTORY_MOMENTS)
    return pt_fail("%s: the current plane has no moments: the lookup was made without PT_HISTORY_MOMENTS (pt_group_history_reproject_ex)", who);
  return 0;
}
// The contexts of a group agree on whether the extra plane E is present (the group's round makes it present in all of them, a clear or
// a move absent; pt_group_context lets a caller break it): the first context that differs from context 0 is the refusal.
int shared_extras(PtGroup* g, const char* who, bool* present) {
  *present = pt_ctx_history_extra_present(g->ctx[0]);
  for (int i = 1; i < g->n; ++i)
    if (pt_ctx_history_extra_present(g->ctx[i]) != *present)
      return pt_fail("%s: context %d %s the extra plane of the history round, context 0 %s it; the contexts of a group share it", who, i,
                     *present ? "does not hold" : "holds", *present ? "holds" : "does not hold");
  return 0;
}
int gather_extra(PtGroup* g) {  // -> g->d_full_extra: W*H floats, the contexts' E planes (all present)
  return gather(g, kExtra, [&](int i) { return pt_ctx_device_history_extra(g->ctx[i]); }, g->d_full_extra);
}
// The end of a call that returns nothing to the host (the capture, the lookup).  COPY transport: the root's stream pulled the tiles out
// of the contexts' buffers, so context i's stream waits until it has before anything that follows (a render, a clear) may overwrite
// them.  RCCL: the sends are on the contexts' own streams already.  (A call that ends in to_host() synchronises everything.)
int release_tiles(PtGroup* g) {
  if (g->transport != PT_GROUP_TRANSPORT_COPY) return 0;
  HIP_OK(hipSetDevice(g->devices[0]));
  if (!g->tiles_read) HIP_OK(hipEventCreateWithFlags(&g->tiles_read, hipEventDisableTiming));
  HIP_OK(hipEventRecord(g->tiles_read, stream(g, 0)));
  for (int i = 1; i < g->n; ++i) {
    HIP_OK(hipSetDevice(g->devices[i]));
    HIP_OK(hipStreamWaitEvent(stream(g, i), g->tiles_read, 0));
  }
  HIP_OK(hipSetDevice(g->devices[0]));
  return 0;
}
// C and VC become absent: pt_group_clear and the moves (K, VK, the kept camera and the kept geoms stay).
void history_current_absent(PtGroup* g) { g->hist_current = false, g->hist_var_current = 0; }

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

// pt_ctx_set_camera on every context; all of them are asked before the first one changes.  The group's own buffers stay.
int pt_group_set_camera(PtGroup* g, const PtCamera* cam) {
  if (!g) return pt_fail("pt_group_set_camera: null group");
  for (PtContext* c : g->ctx)
    if (pt_ctx_camera_refusal(c, cam, "pt_group_set_camera")) return -1;
  history_current_absent(g);  // (the history: as pt_set_camera leaves a context's)
  for (PtContext* c : g->ctx)
    if (pt_ctx_set_camera(c, cam)) return -1;
  return 0;
}

int pt_group_set_geoms(PtGroup* g, const PtGeom* geoms, int num_geoms) {
  if (!g) return pt_fail("pt_group_set_geoms: null group");
  for (PtContext* c : g->ctx)
    if (pt_ctx_geoms_refusal(c, geoms, num_geoms, "pt_group_set_geoms")) return -1;
  history_current_absent(g);
  g->hist_motion.geoms_stale = true, g->hist_motion.fresh = false;  // (the next capture keeps these geoms; K and the kept geoms stay until then)
  for (PtContext* c : g->ctx)
    if (pt_ctx_set_geoms(c, geoms, num_geoms)) return -1;
  return 0;
}

// pt_ctx_set_materials on every context, asked first in the same way; of the group's history K, VK, the kept camera and geoms stay.
int pt_group_set_materials(PtGroup* g, const PtMaterial* materials, int num_materials) {
  if (!g) return pt_fail("pt_group_set_materials: null group");
  for (PtContext* c : g->ctx)
    if (pt_ctx_materials_refusal(c, materials, num_materials, "pt_group_set_materials")) return -1;
  history_current_absent(g);
  for (PtContext* c : g->ctx)
    if (pt_ctx_set_materials(c, materials, num_materials)) return -1;
  return 0;
}

// pt_ctx_clear on every context; the group's buffers stay, and of its history K, VK, the kept camera and the kept geoms.
int pt_group_clear(PtGroup* g) {
  if (!g) return pt_fail("pt_group_clear: null group");
  history_current_absent(g);
  for (PtContext* c : g->ctx)
    if (pt_ctx_clear(c)) return -1;
  return 0;
}
int64_t pt_group_device_bytes(const PtGroup* g) { return g ? g->owned_bytes : 0; }
int pt_group_set_camera_ex(PtGroup* g, const PtCamera* cam, uint32_t flags) {
  if (!g) return pt_fail("pt_group_set_camera_ex: null group");
  for (PtContext* c : g->ctx)
    if (pt_ctx_camera_refusal_ex(c, cam, flags, "pt_group_set_camera_ex")) return -1;
  history_current_absent(g);
  for (PtContext* c : g->ctx)
    if (pt_ctx_set_camera_ex(c, cam, flags)) return -1;
  return 0;
}

int pt_group_gather(PtGroup* g, float* rgb_sum_host) {
  if (!g || !rgb_sum_host) return pt_fail("pt_group_gather: bad argument");
  HIP_OK(hipSetDevice(g->devices[0]));
  if (g->n == 1) return pt_ctx_readback(g->ctx[0], rgb_sum_host);
  if (gather_image(g)) return -1;
  return to_host(g, rgb_sum_host, g->d_full, frame_pixels(g) * 12);
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
  if (need_features(g, "pt_group_gather_features")) return -1;
  HIP_OK(hipSetDevice(g->devices[0]));
  if (g->n == 1) return pt_ctx_readback_features(g->ctx[0], planes_host);
  if (gather_features(g)) return -1;
  return to_host(g, planes_host, g->d_full_feat, PT_FEATURE_PLANES * frame_pixels(g) * 16);
}

// pt_denoise of the whole frame (filter_admit, filter_run): the SUM image and the feature planes meet on the root.
int pt_group_denoise(PtGroup* g, float samples, const PtDenoiseOptions* opt, float* rgb_avg_host) {
  const char* who = "pt_group_denoise";
  if (!g || !rgb_avg_host) return pt_fail("%s: bad argument", who);
  if (g->n == 1) return pt_ctx_denoise(g->ctx[0], samples, opt, rgb_avg_host);
  if (filter_admit(g, who, true)) return -1;
  ptdn::Job j{};
  if (pt_denoise_resolve(who, ptdn::Form::Plain, samples, 0, 0, opt, &j)) return -1;
  return filter_run(g, false, false, rgb_avg_host, [&](hipStream_t root, const float** d_out) {
    return j.f = {g->W, g->H, g->d_full, g->d_full_feat, nullptr}, pt_denoise_launch(root, j, g->d_denoise, d_out);
  });
}

// pt_denoise_guided of the whole frame: as above, and the noise planes meet on the root like the feature planes.  The filter has ONE
// M and T, so the contexts must agree on them (and none may hold unfolded iterations: its own call would be refused).  The conditions
// are checked context by context, so this is not shared_state() behind two loops: a caller who broke the agreement (pt_group_context)
// would meet another first refusal.
int pt_group_denoise_guided(PtGroup* g, const PtDenoiseOptions* opt, float* rgb_avg_host) {
  const char* who = "pt_group_denoise_guided";
  if (!g || !rgb_avg_host) return pt_fail("%s: bad argument", who);
  if (g->n == 1) return pt_ctx_denoise_guided(g->ctx[0], opt, rgb_avg_host);
  if (filter_admit(g, who, true)) return -1;
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
  ptdn::Job j{};
  if (pt_denoise_resolve(who, ptdn::Form::Guided, 0.0f, groups, iters, opt, &j)) return -1;
  return filter_run(g, true, false, rgb_avg_host, [&](hipStream_t root, const float** d_out) {
    return j.f = {g->W, g->H, g->d_full, g->d_full_feat, g->d_full_noise}, pt_denoise_launch(root, j, g->d_denoise, d_out);
  });
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
  for (PtContext* c : g->ctx)  // (before the first group is rendered: the fold would refuse the extras of a history round after it)
    if (pt_ctx_admit_no_extras(c, "pt_group_render_until")) return -1;
  int group = 0;
  if (group_or_batch(g, group_iters, &group)) return -1;
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
  int group = 0;
  if (group_or_batch(g, group_iters, &group)) return -1;
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
  const size_t frame = frame_pixels(g);
  PtCtxState s{};
  if (shared_state(g, "pt_group_gather_adaptive", &s)) return -1;
  if (!s.adaptive) {
    if (pt_group_sync(g)) return -1;
    for (size_t p = 0; p < frame; ++p) counts[2 * p] = (int32_t)std::min<int64_t>(s.iters, INT32_MAX), counts[2 * p + 1] = s.groups;
    return 0;
  }
  HIP_OK(hipSetDevice(g->devices[0]));
  if (gather_counts(g)) return -1;
  return to_host(g, counts, g->d_full_pair, frame * 8);
}

// pt_resolve of the whole frame: every context resolves its own rows; the rows meet like the image (and in its buffers).
int pt_group_resolve(PtGroup* g, float* rgb_avg_host) {
  if (!g || !rgb_avg_host) return pt_fail("pt_group_resolve: bad argument");
  if (g->n == 1) return pt_ctx_resolve(g->ctx[0], rgb_avg_host);
  const size_t frame = frame_pixels(g);
  std::vector<const float*> tiles(g->n, nullptr);
  for (int i = 0; i < g->n; ++i)
    if (pt_ctx_resolve_device(g->ctx[i], &tiles[i])) return -1;
  HIP_OK(hipSetDevice(g->devices[0]));
  if (gather(g, kRgb, [&](int i) { return tiles[i]; }, g->d_full)) return -1;
  return to_host(g, rgb_avg_host, g->d_full, frame * 12);
}

// pt_denoise_adaptive of the whole frame: as pt_group_denoise_guided, and in the adaptive state the count planes meet on the root too
// (the uniform state: the launcher gives every pixel the shared (T, M), as it does for a context).  Refuses what the context's
// function refuses, in its order, each condition over the contexts in turn.
int pt_group_denoise_adaptive(PtGroup* g, const PtDenoiseOptions* opt, float* rgb_avg_host) {
  const char* who = "pt_group_denoise_adaptive";
  if (!g || !rgb_avg_host) return pt_fail("%s: bad argument", who);
  if (g->n == 1) return pt_ctx_denoise_adaptive(g->ctx[0], opt, rgb_avg_host);
  if (filter_admit(g, who, false)) return -1;
  for (PtContext* c : g->ctx)
    if (!pt_ctx_device_noise(c) || pt_ctx_state(c).groups < 1) return pt_fail("%s: nothing has been folded (pt_group_noise_fold)", who);
  for (int i = 0; i < g->n; ++i)
    if (pt_ctx_state(g->ctx[i]).unfolded != 0)
      return pt_fail("%s: context %d has iterations rendered since its last fold; fold first (pt_group_noise_fold)", who, i);
  PtCtxState s{};
  if (shared_state(g, who, &s)) return -1;
  if (s.groups < 2) return pt_fail("%s: %d group(s) folded; a variance needs at least 2 (pt_group_noise_fold after each group of iterations)", who, s.groups);
  if (s.iters > INT32_MAX) return pt_fail("%s: %lld iterations folded: the per-pixel counts are int32", who, (long long)s.iters);
  ptdn::Job j{};
  if (pt_denoise_resolve(who, ptdn::Form::Adaptive, 0.0f, s.groups, s.iters, opt, &j)) return -1;
  return filter_run(g, true, s.adaptive, rgb_avg_host, [&](hipStream_t root, const float** d_out) {
    j.f = {g->W, g->H, g->d_full, g->d_full_feat, g->d_full_noise};
    j.div.cnt = s.adaptive ? reinterpret_cast<const ptad::Cnt*>(g->d_full_pair) : nullptr;
    return pt_denoise_launch(root, j, g->d_denoise, d_out);
  });
}

int pt_group_gather_u8(PtGroup* g, float samples, uint8_t* rgb8_host) {
  if (!g || !rgb8_host) return pt_fail("pt_group_gather_u8: bad argument");
  const size_t frame = frame_pixels(g);
  std::vector<const uint8_t*> tiles(g->n, nullptr);
  for (int i = 0; i < g->n; ++i)  // every device converts its own rows (x mirror is inside a row)
    if (pt_ctx_save_u8_device(g->ctx[i], samples, &tiles[i])) return -1;
  HIP_OK(hipSetDevice(g->devices[0]));
  if (g->n == 1) return to_host(g, rgb8_host, tiles[0], frame * 3);
  if (gather(g, kRgb8, [&](int i) { return tiles[i]; }, g->d_full8)) return -1;
  return to_host(g, rgb8_host, g->d_full8, frame * 3);
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
  const size_t frame = frame_pixels(g);
  for (PtContext* c : g->ctx)  // (before the tiles' buffers are allocated)
    if (pt_ctx_admit_no_extras(c, "pt_group_preview_rgba8")) return -1;
  if (g->d_prev.empty()) g->d_prev.assign(g->n, nullptr);
  for (int i = 0; i < g->n; ++i) {
    HIP_OK(hipSetDevice(g->devices[i]));
    if (ensure(g, i, g->d_prev[i], (size_t)pt_ctx_pixel_count(g->ctx[i]) * 4)) return -1;
    if (pt_ctx_preview_rgba8_device(g->ctx[i], iterations, g->d_prev[i])) return -1;
  }
  HIP_OK(hipSetDevice(g->devices[0]));
  if (g->n == 1) return to_host(g, rgba_host, g->d_prev[0], frame * 4);
  if (gather(g, kRgba8, [&](int i) { return g->d_prev[i]; }, g->d_full_prev)) return -1;
  return to_host(g, rgba_host, g->d_full_prev, frame * 4);
}

// ---- the reprojected history across the group (include/pt_amd.h "history in groups"): after the same calls a group holds what ONE
// renderer of the whole frame holds, bit for bit.  n == 1 forwards to context 0, whose own state it then is.
int pt_group_history_capture_ex(PtGroup* g, float samples, uint32_t flags) {
  const char* who = "pt_group_history_capture_ex";
  if (!g) return pt_fail("%s: null group", who);
  if (g->n == 1) return pt_ctx_history_capture_ex(g->ctx[0], samples, flags);
  if (history_admit(g, who, true, [&] { return pt_history_check_flags(who, flags, false); })) return -1;
  if (pt_history_check_samples(who, samples) || history_not_built(who, flags)) return -1;
  const bool mom = (flags & PT_HISTORY_MOMENTS) != 0;
  bool extras = false;
  if ((mom && history_current_moments(g, who)) || shared_extras(g, who, &extras)) return -1;
  const size_t frame = frame_pixels(g);
  hipStream_t root = stream(g, 0);
  HIP_OK(hipSetDevice(g->devices[0]));
  if (!g->d_hist) {  // the first capture of the group: zeroed like a context's
    if (ensure(g, 0, g->d_hist, pt_history_state_bytes(frame))) return -1;
    HIP_OK(hipMemsetAsync(g->d_hist, 0, pt_history_state_bytes(frame), root));
  }
  if (mom && !g->d_hist_var) {  // ... with moments
    if (ensure(g, 0, g->d_hist_var, pt_history_variance_bytes(frame))) return -1;
    HIP_OK(hipMemsetAsync(g->d_hist_var, 0, pt_history_variance_bytes(frame), root));
  }
  if (gather_image(g) || gather_features(g) || (extras && gather_extra(g))) return -1;
  const pthi::V4* current = current_plane(g);
  const void* current_var = current && mom ? history_var_plane(g, 1) : nullptr;
  const int N = (int)frame;
  const int rc = mom ? (extras ? pt_history_capture_moments_counted_launch(root, N, g->d_full, g->d_full_feat, current, samples, g->d_full_extra, g->d_hist, current_var,
                                                                            history_var_plane(g, 0))
                               : pt_history_capture_moments_launch(root, N, g->d_full, g->d_full_feat, current, samples, g->d_hist, current_var, history_var_plane(g, 0)))
                     : (extras ? pt_history_capture_counted_launch(root, N, g->d_full, g->d_full_feat, current, samples, g->d_full_extra, g->d_hist)
                               : pt_history_capture_launch(root, N, g->d_full, g->d_full_feat, current, samples, g->d_hist));
  if (rc) return fail_after_drain(g);
  if (release_tiles(g)) return -1;
  g->hist_cam = pt_ctx_camera(g->ctx[0]);
  if (PtHistoryMotion& hm = g->hist_motion; hm.geoms_stale) hm.geoms = pt_ctx_geoms(g->ctx[0]), hm.geoms_stale = false, hm.fresh = false;  // retaken only after a pt_group_set_geoms
  g->hist_kept = true;
  g->hist_var_kept = flags;  // a plain capture: kept without moments
  return 0;
}

int pt_group_history_reproject_ex(PtGroup* g, const PtHistoryOptions* opt, uint32_t flags) {
  const char* who = "pt_group_history_reproject_ex";
  if (!g) return pt_fail("%s: null group", who);
  if (g->n == 1) return pt_ctx_history_reproject_ex(g->ctx[0], opt, flags);
  if (history_admit(g, who, true, [&] { return pt_history_check_flags(who, flags, true); })) return -1;
  pthi::Params P{};
  if (pt_history_resolve_options(who, opt, &P) || history_not_built(who, flags)) return -1;
  const bool motion = (flags & PT_HISTORY_MOTION) != 0;
  const uint32_t kind = flags & ~PT_HISTORY_MOTION;  // 0 or PT_HISTORY_MOMENTS
  if (!g->d_hist || !g->hist_kept) return pt_fail("%s: nothing has been captured (pt_group_history_capture_ex)", who);
  if (kind == PT_HISTORY_MOMENTS && (!g->d_hist_var || g->hist_var_kept != PT_HISTORY_MOMENTS))
    return pt_fail("%s: nothing has been captured with moments (pt_group_history_capture_ex with PT_HISTORY_MOMENTS)", who);
  // the per-geom tables are the same for every context: context 0 builds and keeps them on the root device
  const uint8_t* reject = nullptr;
  const float* table = nullptr;
  const uint8_t* table_kind = nullptr;
  int num_geoms = 0;
  if (pt_ctx_history_geom_table(g->ctx[0], false, &reject, &num_geoms)) return -1;
  if (motion && pt_ctx_history_motion_table(g->ctx[0], &g->hist_motion, &table, &table_kind)) return -1;
  hipStream_t root = stream(g, 0);
  HIP_OK(hipSetDevice(g->devices[0]));
  if (gather_features(g)) return -1;
  const pthi::View v = pthi::make_view(g->hist_cam, g->H, 0);
  void* C = history_plane(g, pthi::kKeptPlanes);
  void* VK = kind ? history_var_plane(g, 0) : nullptr;
  void* VC = kind ? history_var_plane(g, 1) : nullptr;
  const int rc = table  ? pt_history_reproject_motion_launch(root, kind, v, g->d_hist, g->d_full_feat, reject, num_geoms, P, C, VK, VC, table, table_kind)
                 : kind ? pt_history_reproject_moments_launch(root, v, g->d_hist, g->d_full_feat, reject, num_geoms, P, C, VK, VC)
                        : pt_history_reproject_launch(root, v, g->d_hist, g->d_full_feat, reject, num_geoms, P, C);
  if (rc) return fail_after_drain(g);
  if (release_tiles(g)) return -1;
  g->hist_current = true;
  g->hist_var_current = kind;
  return 0;
}

int pt_group_history_resolve(PtGroup* g, float samples, float* rgb_avg_host) {
  const char* who = "pt_group_history_resolve";
  if (!g) return pt_fail("%s: null group", who);
  if (g->n == 1) return pt_ctx_history_resolve(g->ctx[0], samples, rgb_avg_host);
  bool extras = false;
  if (history_admit(g, who, false, no_flags) || pt_history_check_samples(who, samples) || shared_extras(g, who, &extras)) return -1;
  if (!rgb_avg_host) return pt_fail("%s: null buffer", who);
  const size_t frame = frame_pixels(g);
  hipStream_t root = stream(g, 0);
  HIP_OK(hipSetDevice(g->devices[0]));
  if (ensure(g, 0, g->d_blend, frame * 12)) return -1;
  if (gather_image(g) || (extras && gather_extra(g))) return -1;
  if (extras ? pt_history_blend_counted_launch(root, (int)frame, g->d_full, samples, g->d_full_extra, current_plane(g), g->d_blend)
             : pt_history_blend_launch(root, (int)frame, g->d_full, samples, current_plane(g), g->d_blend))
    return fail_after_drain(g);
  return to_host(g, rgb_avg_host, g->d_blend, frame * 12);
}

int pt_group_history_denoise_ex(PtGroup* g, float samples, const PtDenoiseOptions* opt, uint32_t flags, float* rgb_avg_host) {
  const char* who = "pt_group_history_denoise_ex";
  if (!g) return pt_fail("%s: null group", who);
  if (g->n == 1) return pt_ctx_history_denoise_ex(g->ctx[0], samples, opt, flags, rgb_avg_host);
  if (history_admit(g, who, true, [&] { return pt_history_check_denoise_flags(who, flags); })) return -1;
  ptdn::Job j{};
  if (pt_history_check_samples(who, samples) || pt_denoise_resolve(who, ptdn::Form::Moments, samples, 0, 0, opt, &j)) return -1;
  if (flags != PT_HISTORY_MOMENTS)
    return pt_fail("%s: the filter with the fold's variance (flags 0, PT_HISTORY_VARIANCE's side) is not built for a group; pass PT_HISTORY_MOMENTS", who);
  bool extras = false;
  if (history_current_moments(g, who) || shared_extras(g, who, &extras)) return -1;
  if (!rgb_avg_host) return pt_fail("%s: null buffer", who);
  const size_t frame = frame_pixels(g);
  HIP_OK(hipSetDevice(g->devices[0]));
  if (ensure(g, 0, g->d_denoise, pt_denoise_workspace_bytes(frame))) return -1;
  if (gather_image(g) || gather_features(g) || (extras && gather_extra(g))) return -1;
  j.f = {g->W, g->H, g->d_full, g->d_full_feat, nullptr};
  if (g->hist_current) {
    j.div.C = reinterpret_cast<const ptdn::V4*>(history_plane(g, pthi::kKeptPlanes));
    j.div.VC = reinterpret_cast<const ptdn::V4*>(history_var_plane(g, 1));
  }
  j.div.E = extras ? g->d_full_extra : nullptr;  // counted: the prepare reads ns = samples + E_p
  const float* d_out = nullptr;
  if (pt_denoise_launch(stream(g, 0), j, g->d_denoise, &d_out)) return fail_after_drain(g);
  return to_host(g, rgb_avg_host, d_out, frame * 12);
}

// The history round: group_round()'s shape with the history's key.  The frame's selection runs once, on the root, over the assembled
// features and the group's C; every context renders and merges its own part (pt_ctx_history_round_list_device).
//
// Buffer order.  d_full_feat, the keys, d_list and d_parts are written and read on the root's stream only, behind the gathers that the
// root's stream ordered after the contexts' feature passes (exchange()).  The read-back synchronises the root's stream, so when a
// context's render begins the root has read that context's feature planes.  The parts go back as scatter_parts() says; context i's
// render and merge are queued on ITS stream behind the copy (or receive) of its part.  The next exchange that reads a context's image
// or E — the resolve, the filter, the capture, the next round — waits for ready[i], recorded on context i's stream behind that merge
// (COPY), or sends on that stream (RCCL); and the group's C, which the key read, is next written by a lookup on the root's stream.
int pt_group_history_round(PtGroup* g, int iter_first, int group_iters, const PtHistoryRoundOptions* opt, int* fresh, int* selected) {
  const char* who = "pt_group_history_round";
  if (!g) return pt_fail("%s: null group", who);
  if (g->n == 1) return pt_ctx_history_round(g->ctx[0], iter_first, group_iters, opt, fresh, selected);
  const int n = g->n, W = g->W, H = g->H;
  const size_t frame = frame_pixels(g);
  for (PtContext* c : g->ctx)
    if (pt_ctx_history_round_refusal(c, who, iter_first, group_iters)) return -1;
  pthi::RoundParams P{};
  bool extras = false;
  if (pt_history_round_options(who, opt, &P) || shared_extras(g, who, &extras) || round_limits(g, who)) return -1;
  const int cap = ptad::list_length((double)P.max_fraction, (int64_t)frame);
  hipStream_t root = stream(g, 0);
  const uint8_t* emitter = nullptr;
  int num_geoms = 0;
  if (pt_ctx_history_geom_table(g->ctx[0], true, &emitter, &num_geoms) || selection_buffers(g)) return -1;

  // collect on the root: the features, key, select, partition
  if (gather_features(g)) return -1;
  if (pt_history_key_launch(root, (int)frame, g->d_full_feat, current_plane(g), emitter, num_geoms, P.min_history, pt_adaptive_select_keys(g->d_select, frame)) ||
      pt_adaptive_select_threshold_keys_launch(root, W, H, 0.0f, cap, g->d_select, g->d_list) ||
      pt_group_partition_launch(root, W, n, g->d_list, pt_adaptive_select_result(g->d_select, frame), cap, g->d_partition, g->d_parts, g->d_result))
    return fail_after_drain(g);

  // read back: fresh, m and the parts' lengths
  std::vector<uint32_t> result;
  if (read_selection(g, who, cap, "fresh", &result)) return -1;
  const int m = (int)result[1];
  if (fresh) *fresh = (int)result[0];
  if (selected) *selected = m;
  if (m == 0) return 0;  // nothing rendered, merged or allocated; E keeps its state

  // distribute and render: part i to context i, on context i's stream; a context with an empty part runs it too, so that all hold E
  if (scatter_parts(g, result.data() + 2)) return -1;
  for (int i = 0; i < n; ++i) {
    const int pixels = pt_ctx_pixel_count(g->ctx[i]);
    if (pt_ctx_history_round_list_device(g->ctx[i], iter_first, group_iters, i == 0 ? g->d_parts : g->d_part[i], (int)result[2 + (size_t)i], cap < pixels ? cap : pixels))
      return fail_after_drain(g);
  }
  return 0;
}

int pt_group_history_drop(PtGroup* g) {
  if (!g) return pt_fail("pt_group_history_drop: null group");
  if (g->n == 1) return pt_ctx_history_drop(g->ctx[0]);
  const size_t frame = frame_pixels(g);
  if (g->d_hist) {  // forgotten, not freed
    HIP_OK(hipSetDevice(g->devices[0]));
    HIP_OK(hipMemsetAsync(g->d_hist, 0, pt_history_state_bytes(frame), stream(g, 0)));
    if (g->d_hist_var) HIP_OK(hipMemsetAsync(g->d_hist_var, 0, pt_history_variance_bytes(frame), stream(g, 0)));
  }
  g->hist_kept = false, g->hist_var_kept = 0;
  history_current_absent(g);
  return 0;
}

int pt_group_readback_history(PtGroup* g, float* kept_planes, float* current_plane_host) {
  const char* who = "pt_group_readback_history";
  if (!g) return pt_fail("%s: null group", who);
  if (g->n == 1) return pt_ctx_readback_history(g->ctx[0], kept_planes, current_plane_host);
  if (!g->d_hist) return pt_fail("%s: nothing has been captured (pt_group_history_capture_ex)", who);
  const size_t frame = frame_pixels(g), plane = frame * sizeof(pthi::V4);
  HIP_OK(hipSetDevice(g->devices[0]));
  if (kept_planes) HIP_OK(hipMemcpyAsync(kept_planes, g->d_hist, pthi::kKeptPlanes * plane, hipMemcpyDeviceToHost, stream(g, 0)));
  if (current_plane_host && g->hist_current) HIP_OK(hipMemcpyAsync(current_plane_host, current_plane(g), plane, hipMemcpyDeviceToHost, stream(g, 0)));
  if (pt_group_sync(g)) return -1;
  if (current_plane_host && !g->hist_current) std::fill(current_plane_host, current_plane_host + 4 * frame, 0.0f);
  return 0;
}

int pt_group_readback_history_variance(PtGroup* g, float* kept_var, float* current_var) {
  if (!g) return pt_fail("pt_group_readback_history_variance: null group");
  if (g->n == 1) return pt_ctx_readback_history_variance(g->ctx[0], kept_var, current_var);
  const size_t frame = frame_pixels(g), plane = frame * sizeof(pthi::V4);
  const bool kept = g->d_hist_var && g->hist_var_kept, current = g->d_hist_var && g->hist_var_current;
  HIP_OK(hipSetDevice(g->devices[0]));
  if (kept_var && kept) HIP_OK(hipMemcpyAsync(kept_var, history_var_plane(g, 0), plane, hipMemcpyDeviceToHost, stream(g, 0)));
  if (current_var && current) HIP_OK(hipMemcpyAsync(current_var, history_var_plane(g, 1), plane, hipMemcpyDeviceToHost, stream(g, 0)));
  if (pt_group_sync(g)) return -1;
  if (kept_var && !kept) std::fill(kept_var, kept_var + 4 * frame, 0.0f);
  if (current_var && !current) std::fill(current_var, current_var + 4 * frame, 0.0f);
  return 0;
}

int pt_group_readback_history_extra(PtGroup* g, float* extra) {
  const char* who = "pt_group_readback_history_extra";
  if (!g) return pt_fail("%s: null group", who);
  if (g->n == 1) return pt_ctx_readback_history_extra(g->ctx[0], extra);
  if (!extra) return pt_fail("%s: null buffer", who);
  bool extras = false;
  if (shared_extras(g, who, &extras)) return -1;
  if (!extras) {
    if (pt_group_sync(g)) return -1;
    std::fill(extra, extra + frame_pixels(g), 0.0f);
    return 0;
  }
  HIP_OK(hipSetDevice(g->devices[0]));
  if (gather_extra(g)) return -1;
  return to_host(g, extra, g->d_full_extra, frame_pixels(g) * sizeof(float));
}

}  // extern "C"
