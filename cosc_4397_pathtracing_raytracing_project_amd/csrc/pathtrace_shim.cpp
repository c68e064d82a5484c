// pathtrace_shim.cpp — the four reference entry points (src/pathtrace.h:6-9)
// implemented over the C ABI.  See include/pathtrace_amd.hpp for the contract.
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/pathtrace_amd.hpp"
#include "pt_scene.h"

extern "C" int pt_preview_rgba8_device(int iterations, void* rgba_dev);

namespace {
pt::Scene* hst_scene = nullptr;
GuiDataContainer* guiData = nullptr;
int q_first = 0, q_count = 0;  // queued, not yet submitted iterations [q_first, q_first+q_count)
int last_iter = 0;
int arith_mode = PT_ARITH_EXACT;
int aa_mode = 0;
int conv_mode = 0;
// pathtraceSetKeepRenderer: a renderer that pathtraceFree() parked instead of freeing, and what it was created from; the next
// pathtraceInit() moves its camera (pt_set_camera) when nothing but the camera differs
int keep_mode = 0;
bool parked = false;
struct Created {
  std::vector<PtGeom> geoms;
  std::vector<PtMaterial> materials;
  int res[2] = {0, 0}, depth = 0, arith = 0, aa = 0, conv = 0;
  bool same_but_camera(const Created& o) const {
    auto equal = [](const auto& a, const auto& b) { return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0]))); };
    return equal(geoms, o.geoms) && equal(materials, o.materials) && res[0] == o.res[0] && res[1] == o.res[1] && depth == o.depth && arith == o.arith &&
           aa == o.aa && conv == o.conv;
  }
} created;

void check(int rc, const char* what) {  // pathtrace.cu:141-150
  if (rc == 0) return;
  std::fprintf(stderr, "HIP error (%s): %s\n", what, pt_last_error());
  std::exit(EXIT_FAILURE);
}
void flush() {
  if (q_count > 0) check(pt_render(q_first, q_count), "pathtrace");
  q_count = 0;
}
}  // namespace

void InitDataContainer(GuiDataContainer* imGuiData) { guiData = imGuiData; }
void pathtraceSetArith(int pt_arith) { arith_mode = pt_arith; }
void pathtraceSetAntialias(int on) { aa_mode = on ? 1 : 0; }
void pathtraceSetConvergence(int n) { conv_mode = n; }
void pathtraceSetKeepRenderer(int on) { keep_mode = on ? 1 : 0; }

void pathtraceInit(pt::Scene* scene) {
  hst_scene = scene;
  PtSceneDesc d = scene->desc();
  PtOptions opt{};
  opt.arith = arith_mode;
  opt.aa_jitter = aa_mode;
  opt.convergence = conv_mode;
  q_count = 0;
  last_iter = 0;
  const bool was_parked = parked;
  parked = false;
  if (keep_mode || was_parked) {
    Created now;
    now.geoms = scene->geoms, now.materials = scene->materials;
    now.res[0] = d.camera.resolution[0], now.res[1] = d.camera.resolution[1];
    now.depth = d.trace_depth, now.arith = arith_mode, now.aa = aa_mode, now.conv = conv_mode;
    if (was_parked && keep_mode && now.same_but_camera(created)) {  // the camchanged case: the renderer stays, its camera moves
      check(pt_set_camera(&d.camera), "pathtraceInit (pt_set_camera)");
      return;
    }
    created = std::move(now);
  }
  check(pt_init(&d, &opt), "pathtraceInit");  // (frees a parked renderer first)
}

void pathtraceSyncImage() {
  if (!hst_scene) return;
  flush();
  const PtCamera& c = hst_scene->state.camera;
  hst_scene->state.image.resize((size_t)c.resolution[0] * c.resolution[1] * 3);
  check(pt_readback(hst_scene->state.image.data()), "pathtraceSyncImage");
}

void pathtraceFree() {
  if (hst_scene && last_iter > 0) pathtraceSyncImage();
  if (keep_mode && hst_scene) parked = true;  // the image is read back as always; the renderer waits for the next pathtraceInit()
  else if (!(keep_mode && parked)) {  // (a second pathtraceFree() leaves a parked renderer parked)
    check(pt_free(), "pathtraceFree");
    parked = false;
  }
  hst_scene = nullptr;
  q_count = 0;
  last_iter = 0;
}

void pathtraceShutdown() {
  pathtraceFree();
  parked = false;
  check(pt_free(), "pathtraceShutdown");
  created = Created{};
}

void pathtrace(pt_uchar4* pbo, int /*frame*/, int iter) {
  if (!hst_scene) {
    std::fprintf(stderr, "pathtrace() before pathtraceInit()\n");
    std::exit(EXIT_FAILURE);
  }
  if (q_count > 0 && iter != q_first + q_count) flush();
  if (q_count == 0) q_first = iter;
  ++q_count;
  last_iter = iter;
  if (guiData) guiData->TracedDepth = hst_scene->state.traceDepth;
  const bool final_iter = iter >= (int)hst_scene->state.iterations;
  if (pbo) {
    flush();
    check(pt_preview_rgba8_device(iter, pbo), "sendImageToPBO");
  }
  if (final_iter || q_count >= 64) flush();
  if (final_iter) pathtraceSyncImage();
}

float pathtracePSNR(int iter) {  // what pathtrace.cu:627-638 prints after iteration `iter`
  if (!hst_scene) return FLT_MAX;
  flush();
  double sse = -1.0;
  check(pt_get_convergence(iter, 1, &sse), "pathtracePSNR");
  const PtCamera& c = hst_scene->state.camera;
  return sse < 0.0 ? FLT_MAX : pt_psnr_from_sse(sse, (int64_t)c.resolution[0] * c.resolution[1]);
}
