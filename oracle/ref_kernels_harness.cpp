// oracle/ref_kernels_harness.cpp — TEST INFRASTRUCTURE ONLY (golden generation).
//
// Pins the last part of the reference that was held by whole-image known answers only, to the reference's OWN text:
//   * the __global__ bodies of src/pathtrace.cu — generateRayFromCamera :270-286, computeIntersections :288-333,
//     shadeAndExtendRays :336-437, finalGather :439-444 — with what they call (BVH structs and intersectAABB :23-128,
//     MAX_MATERIALS :138, makeSeededRandomEngine :203-207, the sampling helpers :208-248);
//   * main.cpp's camera fix-up: the statement sequences :57-71 (orbit state from the loaded camera) and :110-128 (the
//     `camchanged` block of runCuda()).
// The Makefile cuts those line ranges out of the two files AT BUILD TIME into a scratch directory under /tmp (never into this
// repository, never onto the GPU box); this harness includes them from there.  Nothing of the reference is copied into the
// repository; the fixtures hold numbers only.
//
// Stand-ins for the CUDA toolchain (all of them here, none in the included text):
//   * threadIdx / blockIdx / blockDim are macros naming three plain structs of this file (the genuine <cuda_runtime.h>
//     declares the real ones `const`); a kernel body is called once per thread with blockDim = 1 and blockIdx = the index;
//   * __global__ and __shared__ are redefined empty AFTER the reference's headers; __syncthreads() is an empty function;
//   * `Material sharedMat[MAX_MATERIALS]` at namespace scope satisfies shadeAndExtendRays' block-scope extern declaration;
//   * `namespace thrust` forwards default_random_engine and uniform_real_distribution<float> to rocThrust's own, compiled in
//     ref_kernels_thrust.cpp (the reference's CUDA Thrust is not vendored; rocThrust is the same published algorithm, pinned on
//     its own by ref_rng_harness.cpp).  The distribution's (0.0f, 1.0f) bounds are fixed there, as pathtrace.cu:369 passes them;
//   * the file-scope variables of main.cpp that the two statement sequences use are declared here with main.cpp's types.
//
// What remains RESTATED after this, and lives in this file:
//   * the launch order of pathtrace() (the host loop).  renderSum() below is this harness's own loop:
//       generateRayFromCamera over all pixels                     pathtrace.cu:544
//       per depth < traceDepth:                                   pathtrace.cu:561
//         memset of the intersection buffer                       pathtrace.cu:562
//         computeIntersections over all pixels                    pathtrace.cu:567  (num_paths stays pixelcount: no compaction)
//         shadeAndExtendRays over all pixels                      pathtrace.cu:584
//       finalGather                                               pathtrace.cu:610
//     with the image zeroed once before the first iteration (pathtraceInit, pathtrace.cu:469) and iterations counted from 1
//     (main.cpp:140);
//   * the mouse callbacks (main.cpp:192-199), whose increments are double-precision expressions of cursor positions:
//     pt_scene_orbit replaces them by a float rule of its own (phi += dphi; theta = fmax(0.001f, fmin(theta + dtheta, PI));
//     zoom = fmax(0.1f, zoom + dzoom)), and the `camera` mode makes its states by that rule — only the block that turns a
//     state into a camera is the reference's text.
//
// Modes (a comma-separated list selects several; every mode adds sections to the one output file):
//   ref_kernels MODES OUT.bin ISECT.bin SHADE_SCENE.txt CORNELL.txt SPHERE.txt TWISTED.txt QUIRKS.txt
//     camera     per scene: the loader's camera, the orbit state after :57-71, the camera after :110-128; then the block on a
//                list of states reached by float drags (both clamps' edges, a zero drag, a full turn in 16 steps)
//     generate   generateRayFromCamera for every pixel of small frames (odd, non-square, cornell's square frame whose
//                diagonals look along the box's edges)
//     intersect  computeIntersections' full record for the rays of ISECT.bin (ref_hot's sets 0 and 1: CORNELL, TWISTED)
//     shade      one shadeAndExtendRays call per vector on SHADE_SCENE's materials, with a count per branch reached
//     images     the SUM image after renderSum()
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>
#include <unistd.h>
#include <vector>
using std::max;  // CUDA's global min()/max() overloads exist only under nvcc (intersections.h:131,134)
using std::min;

#include "sceneStructs.h"
#include "scene.h"
#include "glm/glm.hpp"
#include "glm/gtx/norm.hpp"
#include "utilities.h"
#include "intersections.h"

#include "ref_gold_io.h"

// ───────────────────────── stand-ins (see the header) ─────────────────────────
struct RefDim3 {
  unsigned x, y, z;
};
static RefDim3 ref_threadIdx = {0, 0, 0}, ref_blockIdx = {0, 0, 0}, ref_blockDim = {1, 1, 1};
#define threadIdx ref_threadIdx
#define blockIdx ref_blockIdx
#define blockDim ref_blockDim
#undef __global__
#define __global__
#undef __shared__
#define __shared__
static inline void __syncthreads() {}

extern "C" {
void ref_thrust_seed(void* storage16, int h);
unsigned ref_thrust_next(void* storage16);
float ref_thrust_u01(void* storage16);
}
namespace thrust {
struct default_random_engine {
  alignas(8) unsigned char storage[16];
  default_random_engine(int h) { ref_thrust_seed(storage, h); }
  unsigned operator()() { return ref_thrust_next(storage); }
};
template <typename T>
struct uniform_real_distribution {
  uniform_real_distribution(T, T) {}
  T operator()(default_random_engine& e) { return ref_thrust_u01(e.storage); }
};
}  // namespace thrust

#include "ref_k_bvh.inc"      // src/pathtrace.cu:23-128, cut out at build time (oracle/Makefile)
#include "ref_k_maxmat.inc"   // src/pathtrace.cu:138
#include "ref_k_seed.inc"     // src/pathtrace.cu:203-207
#include "ref_k_helpers.inc"  // src/pathtrace.cu:208-248
Material sharedMat[MAX_MATERIALS];
#include "ref_k_kernels.inc"  // src/pathtrace.cu:270-444

// main.cpp's file-scope variables (main.cpp:14,18-20,24-25), used by the two statement sequences
static bool camchanged = true;
float zoom, theta, phi;
glm::vec3 cameraPosition;
glm::vec3 ogLookAt;
RenderState* renderState;
int iteration;

static void mainCameraSetup() {  // main.cpp:53 binds `cam`; :57-71 follow
  Camera& cam = renderState->camera;
#include "ref_main_setup.inc"  // src/main.cpp:57-71
}
static void runCudaCameraBlock() {
#include "ref_main_camchanged.inc"  // src/main.cpp:110-128
}

using gold::bitsf;
using gold::fbits;

// ───────────────────────── our own plumbing ─────────────────────────
static void putVec(std::vector<uint32_t>& w, const glm::vec3& v) {
  w.push_back(fbits(v.x));
  w.push_back(fbits(v.y));
  w.push_back(fbits(v.z));
}
static void putCamera(std::vector<uint32_t>& w, const Camera& c) {  // the field order of PtCamera / OrcCamera: 21 words
  w.push_back((uint32_t)c.resolution.x), w.push_back((uint32_t)c.resolution.y);
  putVec(w, c.position), putVec(w, c.lookAt), putVec(w, c.view), putVec(w, c.up), putVec(w, c.right);
  w.push_back(fbits(c.fov.x)), w.push_back(fbits(c.fov.y));
  w.push_back(fbits(c.pixelLength.x)), w.push_back(fbits(c.pixelLength.y));
}

// new Scene(path) as main.cpp:45 does.  For a frame of another size the scene text is copied to a scratch file with its RES
// line replaced, so that the loader itself computes fov and pixelLength (scene.cpp:133-140); the copy is removed at once.
static Scene* loadScene(const char* path, int w, int h) {
  if (w <= 0) return new Scene(path);  // never deleted: scene.h:21 declares a destructor scene.cpp never defines
  std::ifstream in(path);
  if (!in.is_open()) {
    fprintf(stderr, "ref_kernels: cannot read %s\n", path);
    exit(1);
  }
  char tmp[96];
  snprintf(tmp, sizeof tmp, "/tmp/ref_kernels_scene_%d.txt", (int)getpid());
  {
    std::ofstream out(tmp);
    std::string line;
    while (std::getline(in, line)) {
      if (line.compare(0, 3, "RES") == 0 && line.size() > 3 && (line[3] == ' ' || line[3] == '\t'))
        out << "RES         " << w << " " << h << "\n";
      else
        out << line << "\n";
    }
  }
  Scene* s = new Scene(tmp);
  remove(tmp);
  return s;
}

// main() up to the first pathtrace(): state from the loaded camera, then the first runCuda() with camchanged == true
static void startViewer(Scene* scene) {
  iteration = 0;
  renderState = &scene->state;
  mainCameraSetup();
  camchanged = true;
  runCudaCameraBlock();
}

// ───────────────────────── camera ─────────────────────────
static void modeCamera(gold::File& f, char** scenes, int nscenes) {
  gold::Section& loaded = f.add("cam_loaded", 21);
  gold::Section& state0 = f.add("cam_state0", 9);  // phi, theta, zoom, cameraPosition, ogLookAt after main.cpp:57-71
  gold::Section& fixed = f.add("cam_fixed", 21);
  // drags (dphi, dtheta, dzoom), applied in sequence from the loaded scene by pt_scene_orbit's float rule
  std::vector<glm::vec3> drags;
  drags.push_back(glm::vec3(0.0f));                                              // nothing
  for (int k = 0; k < 16; ++k) drags.push_back(glm::vec3(6.2831853071795864769f / 16.0f, 0.0f, 0.0f));  // a full turn
  drags.push_back(glm::vec3(0.5f, -0.25f, 2.0f));
  drags.push_back(glm::vec3(0.0f, 10.0f, 0.0f));    // theta clamps at PI
  drags.push_back(glm::vec3(0.3f, 0.0f, 0.0f));     // turning at the clamp
  drags.push_back(glm::vec3(0.0f, 0.0f, 0.0f));
  drags.push_back(glm::vec3(0.0f, -10.0f, 0.0f));   // theta clamps at 0.001
  drags.push_back(glm::vec3(-1.7f, 0.0f, 0.5f));
  drags.push_back(glm::vec3(0.0f, 0.001f, 0.0f));   // just off the edge
  drags.push_back(glm::vec3(0.0f, 1.25f, -100.0f)); // zoom clamps at 0.1
  drags.push_back(glm::vec3(0.1f, 0.5f, 0.0f));     // moving at the smallest zoom
  drags.push_back(glm::vec3(0.0f, 0.0f, 0.0f));
  drags.push_back(glm::vec3(0.0f, 0.0f, 7.25f));
  drags.push_back(glm::vec3(-9.0f, -0.6f, 3.0f));   // phi far outside [0, 2 PI]
  drags.push_back(glm::vec3(100.0f, 0.1f, 0.0f));
  drags.push_back(glm::vec3(1e-6f, -1e-6f, 1e-6f));
  const float pi = PI;  // utilities.h:12
  for (int s = 0; s < nscenes; ++s) {
    Scene* scene = loadScene(scenes[s], 0, 0);
    putCamera(loaded.w, scene->state.camera);
    iteration = 0;
    renderState = &scene->state;
    mainCameraSetup();
    state0.w.push_back(fbits(phi)), state0.w.push_back(fbits(theta)), state0.w.push_back(fbits(zoom));
    putVec(state0.w, cameraPosition), putVec(state0.w, ogLookAt);
    camchanged = true;
    runCudaCameraBlock();
    putCamera(fixed.w, scene->state.camera);
    char name[24];
    snprintf(name, sizeof name, "orbit_%d", s);  // drag, state reached, camera after the camchanged block
    gold::Section& ob = f.add(name, 3 + 3 + 21);
    for (const glm::vec3& d : drags) {
      phi += d.x;
      theta = fmaxf(0.001f, fminf(theta + d.y, pi));
      zoom = fmaxf(0.1f, zoom + d.z);
      camchanged = true;
      runCudaCameraBlock();
      putVec(ob.w, d);
      ob.w.push_back(fbits(phi)), ob.w.push_back(fbits(theta)), ob.w.push_back(fbits(zoom));
      putCamera(ob.w, scene->state.camera);
    }
  }
}

// ───────────────────────── generate ─────────────────────────
static void runGenerate(const Camera& cam, int iter, int traceDepth, std::vector<PathSegment>& paths) {
  for (int y = 0; y < cam.resolution.y; ++y)
    for (int x = 0; x < cam.resolution.x; ++x) {
      ref_blockIdx.x = (unsigned)x, ref_blockIdx.y = (unsigned)y;
      generateRayFromCamera(cam, iter, traceDepth, paths.data());
    }
  ref_blockIdx.x = ref_blockIdx.y = 0;
}

static int modeGenerate(gold::File& f, char** scenes) {
  // scene, width, height
  const int frames[][3] = {{0, 61, 37}, {0, 32, 32}, {0, 48, 32}, {1, 24, 16}, {1, 17, 23}, {2, 24, 16}, {2, 17, 23}, {3, 24, 16}, {3, 17, 23}};
  gold::Section& fr = f.add("gen_frames", 4);  // scene, width, height, traceDepth
  int k = 0;
  for (const auto& q : frames) {
    Scene* scene = loadScene(scenes[q[0]], q[1], q[2]);
    startViewer(scene);
    const Camera& cam = scene->state.camera;
    const int n = cam.resolution.x * cam.resolution.y;
    std::vector<PathSegment> paths(n);
    memset(paths.data(), 0xff, n * sizeof(PathSegment));
    runGenerate(cam, 1, scene->state.traceDepth, paths);
    fr.w.push_back((uint32_t)q[0]), fr.w.push_back((uint32_t)q[1]), fr.w.push_back((uint32_t)q[2]);
    fr.w.push_back((uint32_t)scene->state.traceDepth);
    char name[24];
    snprintf(name, sizeof name, "gen_%d", k++);  // origin, direction, colour, pixelIndex, remainingBounces per pixel
    gold::Section& g = f.add(name, 11);
    for (int i = 0; i < n; ++i) {
      putVec(g.w, paths[i].ray.origin), putVec(g.w, paths[i].ray.direction), putVec(g.w, paths[i].color);
      g.w.push_back((uint32_t)paths[i].pixelIndex), g.w.push_back((uint32_t)paths[i].remainingBounces);
    }
  }
  return 0;
}

// ───────────────────────── intersect ─────────────────────────
static void runIntersect(int depth, Scene* scene, std::vector<BVHNodeGPU>& nodes, std::vector<PathSegment>& paths,
                         std::vector<ShadeableIntersection>& isects) {
  const int n = (int)paths.size();
  for (int i = 0; i < n; ++i) {
    ref_blockIdx.x = (unsigned)i;
    computeIntersections(depth, n, paths.data(), scene->geoms.data(), (int)scene->geoms.size(), isects.data(), nodes.data());
  }
  ref_blockIdx.x = 0;
}

static int modeIntersect(gold::File& f, const char* isect, char** scenes) {
  gold::File in;
  if (!in.read(isect)) return 1;
  const int which[2] = {0, 2};  // ref_hot's set 0 = CORNELL, set 1 = TWISTED
  gold::Section& sets = f.add("isect_sets", 2);  // scene, rays
  for (int s = 0; s < 2; ++s) {
    Scene* scene = loadScene(scenes[which[s]], 0, 0);
    std::vector<BVHNodeGPU> nodes;
    buildBVH(scene->geoms, nodes);
    char name[24];
    snprintf(name, sizeof name, "rays_%d", s);
    const gold::Section* rs = in.find(name);
    if (!rs || rs->cols != 6) return 1;
    std::vector<PathSegment> paths(rs->rows);
    for (uint32_t r = 0; r < rs->rows; ++r) {
      const uint32_t* w = rs->w.data() + 6 * (size_t)r;
      paths[r].ray.origin = glm::vec3(bitsf(w[0]), bitsf(w[1]), bitsf(w[2]));
      paths[r].ray.direction = glm::vec3(bitsf(w[3]), bitsf(w[4]), bitsf(w[5]));
      paths[r].color = glm::vec3(1.0f), paths[r].pixelIndex = (int)r, paths[r].remainingBounces = 1;
    }
    std::vector<ShadeableIntersection> isects(rs->rows);
    memset(isects.data(), 0, isects.size() * sizeof(ShadeableIntersection));  // pathtrace.cu:562
    runIntersect(0, scene, nodes, paths, isects);
    sets.w.push_back((uint32_t)which[s]), sets.w.push_back(rs->rows);
    snprintf(name, sizeof name, "isect_%d", s);  // t, normal, materialId, point, outsideObject, geomIndex
    gold::Section& o = f.add(name, 10);
    for (const ShadeableIntersection& h : isects) {
      o.w.push_back(fbits(h.t));
      putVec(o.w, h.surfaceNormal);
      o.w.push_back((uint32_t)h.materialId);
      putVec(o.w, h.point);
      o.w.push_back(h.outsideObject ? 1u : 0u), o.w.push_back((uint32_t)h.geomIndex);
    }
  }
  return 0;
}

// ───────────────────────── shade ─────────────────────────
// our own input generator (inputs only)
struct Rng {
  uint32_t s;
  explicit Rng(uint32_t seed) : s(seed ? seed : 1u) {}
  uint32_t next() {
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return s;
  }
  float u() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }
  float sym() { return 2.0f * u() - 1.0f; }
  glm::vec3 unit() {
    for (;;) {
      glm::vec3 v(sym(), sym(), sym());
      float l2 = glm::dot(v, v);
      if (l2 > 1e-3f && l2 <= 1.0f) return glm::normalize(v);
    }
  }
};

// The branches a vector is counted under (bit numbers of the two-word mask; tests/test_ref_kernel_goldens.py names them in
// the same order).  Which branch a vector takes is worked out HERE from its inputs and the engine's draws, in the order the
// kernel consumes them; it labels the vectors and decides nothing about the recorded outputs, which are the kernel's.
enum Branch {
  B_MISS_LIVE, B_MISS_DEAD, B_HIT_DEAD, B_EMITTER, B_EMITTER_REFLECTIVE, B_KILL_D4, B_PASS_D4, B_KILL_D63, B_PASS_D63,
  B_SCATTER_D3, B_LOBE_SPECULAR_R03, B_LOBE_DIFFUSE_R03, B_PURE_MIRROR, B_ROUGH_MIRROR, B_DIFFUSE_X_GT_Y, B_DIFFUSE_X_LE_Y,
  B_AXIS_PX, B_AXIS_NX, B_AXIS_PY, B_AXIS_NY, B_AXIS_PZ, B_AXIS_NZ, B_NEG_ZERO_NORMAL, B_LAST_BOUNCE_SCATTERS, B_ZERO_COLOUR_IN,
  B_ITER_1, B_ITER_4194303, B_ITER_4194304, B_ITER_2147483647, B_IDX_LAST_PIXEL, B_MAX_EXACTLY_1_PASS, B_ROUGH_FRAME_X_GT_Y,
  B_ROUGH_FRAME_X_LE_Y, B_IDX_ABOVE_2_20, B_COUNT
};

struct ShadeVec {
  int iter, depth, idx, remaining;
  ShadeableIntersection hit;
  PathSegment seg;
};

static uint64_t classify(const ShadeVec& v, const std::vector<Material>& mats) {
  uint64_t m = 0;
  auto set = [&](int b) { m |= (uint64_t)1 << b; };
  if (v.seg.color.x == 0.0f && v.seg.color.y == 0.0f && v.seg.color.z == 0.0f) set(B_ZERO_COLOUR_IN);
  if (v.hit.t < 0.0f) {
    set(v.remaining > 0 ? B_MISS_LIVE : B_MISS_DEAD);
    return m;
  }
  if (v.remaining <= 0) {
    set(B_HIT_DEAD);
    return m;
  }
  const Material& mat = mats[v.hit.materialId];
  if (mat.emittance > 0.0f) {
    set(mat.hasReflective > 0.0f ? B_EMITTER_REFLECTIVE : B_EMITTER);
    return m;
  }
  thrust::default_random_engine rng = makeSeededRandomEngine(v.iter, v.idx, v.depth);
  thrust::uniform_real_distribution<float> u01(0.0f, 1.0f);
  if (v.iter == 1) set(B_ITER_1);
  if (v.iter == 4194303) set(B_ITER_4194303);
  if (v.iter == 4194304) set(B_ITER_4194304);
  if (v.iter == 2147483647) set(B_ITER_2147483647);
  if (v.idx == 1920 * 1080 - 1) set(B_IDX_LAST_PIXEL);
  if (v.idx > (1 << 20)) set(B_IDX_ABOVE_2_20);
  if (v.depth > 3) {
    const float p = fmaxf(mat.color.x, fmaxf(mat.color.y, mat.color.z));
    const bool killed = u01(rng) > p;
    if (v.depth == 4) set(killed ? B_KILL_D4 : B_PASS_D4);
    if (v.depth == 63) set(killed ? B_KILL_D63 : B_PASS_D63);
    if (killed) return m;
    if (p == 1.0f) set(B_MAX_EXACTLY_1_PASS);
  }
  if (v.depth == 3) set(B_SCATTER_D3);
  if (v.remaining == 1) set(B_LAST_BOUNCE_SCATTERS);
  const glm::vec3 n = v.hit.surfaceNormal;
  if (mat.hasReflective > 0.0f && u01(rng) < mat.hasReflective) {
    if (mat.hasReflective == 0.3f) set(B_LOBE_SPECULAR_R03);
    if (1.0f - mat.hasRefractive > 0.0f) {
      set(B_ROUGH_MIRROR);
      const glm::vec3 r = reflect(v.seg.ray.direction, n);
      set(fabsf(r.x) > fabsf(r.y) ? B_ROUGH_FRAME_X_GT_Y : B_ROUGH_FRAME_X_LE_Y);
    } else {
      set(B_PURE_MIRROR);
    }
    return m;
  }
  if (mat.hasReflective == 0.3f) set(B_LOBE_DIFFUSE_R03);
  set(fabsf(n.x) > fabsf(n.y) ? B_DIFFUSE_X_GT_Y : B_DIFFUSE_X_LE_Y);
  const bool negzero = (n.x == 0.0f && std::signbit(n.x)) || (n.y == 0.0f && std::signbit(n.y)) || (n.z == 0.0f && std::signbit(n.z));
  if (negzero) set(B_NEG_ZERO_NORMAL);
  const int zeros = (n.x == 0.0f) + (n.y == 0.0f) + (n.z == 0.0f);
  if (zeros == 2 && !negzero) {
    if (n.x == 1.0f) set(B_AXIS_PX);
    if (n.x == -1.0f) set(B_AXIS_NX);
    if (n.y == 1.0f) set(B_AXIS_PY);
    if (n.y == -1.0f) set(B_AXIS_NY);
    if (n.z == 1.0f) set(B_AXIS_PZ);
    if (n.z == -1.0f) set(B_AXIS_NZ);
  }
  return m;
}

static void runShade(int iter, int depth, int idx, ShadeableIntersection& hit, PathSegment& seg, std::vector<Material>& mats) {
  // the kernel indexes both arrays with idx (:352-353) and seeds the engine with it (:368): arrays of a 1920 x 1080 frame,
  // the one record of the call at element idx
  static std::vector<ShadeableIntersection> isects(1920 * 1080);
  static std::vector<PathSegment> paths(1920 * 1080);
  isects[idx] = hit, paths[idx] = seg;
  ref_blockIdx.x = (unsigned)idx;
  shadeAndExtendRays(iter, depth, 1920 * 1080, isects.data(), paths.data(), mats.data(), (int)mats.size(), nullptr, 0);
  ref_blockIdx.x = 0;
  hit = isects[idx], seg = paths[idx];
}

static int modeShade(gold::File& f, const char* shadeScene) {
  Scene* scene = loadScene(shadeScene, 0, 0);
  std::vector<Material>& mats = scene->materials;
  const int M = (int)mats.size();
  if (M < 12 || M > MAX_MATERIALS) return 1;
  Rng rng(0x7f4a7c15u);
  std::vector<glm::vec3> axis = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
  std::vector<glm::vec3> negz = {{-0.0f, 1, 0}, {0.6f, -0.0f, 0.8f}, {-0.0f, 0.6f, -0.8f}, {0.8f, -0.6f, -0.0f}, {0, -0.0f, -1}};
  std::vector<glm::vec3> general, dirs, points, colours;
  general.push_back(glm::normalize(glm::vec3(1.0f, 1.0f, 0.0f)));  // |x| == |y|
  general.push_back(glm::normalize(glm::vec3(-1.0f, 1.0f, 1.0f)));
  while (general.size() < 20) general.push_back(rng.unit());
  dirs.push_back(glm::vec3(0, -1, 0)), dirs.push_back(glm::vec3(0, 0, -1)), dirs.push_back(glm::vec3(1, 0, 0));
  dirs.push_back(glm::normalize(glm::vec3(1.0f, -1.0f, 0.0f)));
  while (dirs.size() < 40) dirs.push_back(rng.unit());
  while (points.size() < 24) points.push_back(glm::vec3(5.0f * rng.sym(), 5.0f + 5.0f * rng.sym(), 5.0f * rng.sym()));
  colours = {{1, 1, 1}, {0, 0, 0}, {0.5f, 0.25f, 0.125f}, {0.9f, 0.8f, 0.7f}, {1, 1, 1}, {2.5f, 0.0f, 1e-20f}};
  while (colours.size() < 10) colours.push_back(glm::vec3(rng.u(), rng.u(), rng.u()));
  const int iters[] = {1, 4194303, 4194304, 2147483647, 2, 17, 5000};
  const int fixedIdx[] = {0, 1, 63, 64, 1920 * 1080 - 1, 1920 * 1080 - 1, 1920 * 1080 - 2, 1 << 20, (1 << 20) + 1, 65535, 65536};
  // (depth, remainingBounces, repetitions per material).  remaining = 0 rows are the "nothing changes" returns; a live path of
  // the reference has remaining = traceDepth - depth, so every row with remaining > 0 is a (depth, traceDepth) pair a stage
  // test can set up.  Depths 4 and 63 carry more repetitions: the roulette's two outcomes are counted there.
  const int plan[][3] = {{0, 1, 8}, {0, 3, 8}, {1, 3, 8}, {3, 1, 10}, {3, 5, 10}, {4, 1, 16}, {4, 4, 16}, {5, 3, 8}, {63, 1, 30}, {2, 0, 5}, {4, 0, 5}};
  std::vector<ShadeVec> vecs;
  for (const auto& p : plan) {
    const int depth = p[0], remaining = p[1], reps = p[2];
    for (int pass = 0; pass < 2; ++pass) {  // 0: hits on every material, 1: misses
      const int count = pass == 0 ? M * reps : std::max(60, 3 * reps);
      for (int k = 0; k < count; ++k) {
        ShadeVec v;
        memset(&v, 0, sizeof v);
        v.iter = iters[rng.next() % 7u];
        v.depth = depth;
        v.idx = (rng.next() & 1u) ? fixedIdx[rng.next() % 11u] : (int)(rng.next() % (1920u * 1080u));
        v.remaining = remaining;
        const uint32_t pick = rng.next() % 12u;
        const glm::vec3 n = pick < 6 ? axis[pick] : pick < 8 ? negz[rng.next() % negz.size()] : general[rng.next() % general.size()];
        if (pass == 0) {
          v.hit.t = 0.25f * (float)(1 + rng.next() % 40u);
          v.hit.surfaceNormal = n;
          v.hit.materialId = k % M;
          v.hit.point = points[rng.next() % points.size()];
          v.hit.outsideObject = true;
          v.hit.geomIndex = (int)(rng.next() % 7u);
        } else {
          v.hit.t = -1.0f;  // the rest of the record as the memset leaves it (pathtrace.cu:562)
        }
        v.seg.ray.origin = points[rng.next() % points.size()];
        v.seg.ray.direction = dirs[rng.next() % dirs.size()];
        v.seg.color = colours[rng.next() % colours.size()];
        v.seg.pixelIndex = v.idx;
        v.seg.remainingBounces = remaining;
        vecs.push_back(v);
      }
    }
  }
  gold::Section& in = f.add("shade_in", 21);    // iter, depth, idx, remaining, t, normal, materialId, point, origin, direction, colour
  gold::Section& out = f.add("shade_out", 13);  // origin, direction, colour, remaining, colour after the replayed depths
  gold::Section& br = f.add("shade_branch", 2); // branch mask, low and high word
  std::vector<uint32_t> counts(B_COUNT, 0u);
  for (const ShadeVec& v : vecs) {
    const uint64_t mask = classify(v, mats);
    for (int b = 0; b < B_COUNT; ++b)
      if (mask >> b & 1) counts[b]++;
    in.w.push_back((uint32_t)v.iter), in.w.push_back((uint32_t)v.depth), in.w.push_back((uint32_t)v.idx), in.w.push_back((uint32_t)v.remaining);
    in.w.push_back(fbits(v.hit.t));
    putVec(in.w, v.hit.surfaceNormal);
    in.w.push_back((uint32_t)v.hit.materialId);
    putVec(in.w, v.hit.point), putVec(in.w, v.seg.ray.origin), putVec(in.w, v.seg.ray.direction), putVec(in.w, v.seg.color);
    ShadeableIntersection hit = v.hit;
    PathSegment seg = v.seg;
    runShade(v.iter, v.depth, v.idx, hit, seg, mats);
    putVec(out.w, seg.ray.origin), putVec(out.w, seg.ray.direction), putVec(out.w, seg.color);
    out.w.push_back((uint32_t)seg.remainingBounces);
    // a path that missed stays in the reference's arrays and meets the same miss at every later depth of the loop
    // (pathtrace.cu:561-603: no compaction); with remaining = traceDepth - depth that is remaining - 1 further calls
    if (v.hit.t < 0.0f)
      for (int d = v.depth + 1; d < v.depth + v.remaining; ++d) runShade(v.iter, d, v.idx, hit, seg, mats);
    putVec(out.w, seg.color);
    br.w.push_back((uint32_t)(mask & 0xffffffffu)), br.w.push_back((uint32_t)(mask >> 32));
  }
  gold::Section& cs = f.add("shade_counts", 1);
  bool ok = true;
  for (int b = 0; b < B_COUNT; ++b) {
    cs.w.push_back(counts[b]);
    if (counts[b] < 50) fprintf(stderr, "ref_kernels shade: branch %d reached by %u vectors only\n", b, counts[b]), ok = false;
  }
  return ok ? 0 : 1;
}

// ───────────────────────── images ─────────────────────────
// This harness's own restatement of pathtrace()'s launch order (see the header): the SUM image of iterations
// [first, first + count) at `depth`, the image zeroed before the first of them.
static std::vector<glm::vec3> renderSum(Scene* scene, int depthMax, int first, int count) {
  const Camera& cam = scene->state.camera;
  const int n = cam.resolution.x * cam.resolution.y;
  std::vector<BVHNodeGPU> nodes;
  buildBVH(scene->geoms, nodes);  // pathtraceInit, pathtrace.cu:485
  std::vector<glm::vec3> image(n, glm::vec3(0.0f));  // pathtrace.cu:469
  std::vector<PathSegment> paths(n);
  std::vector<ShadeableIntersection> isects(n);
  for (int iter = first; iter < first + count; ++iter) {
    runGenerate(cam, iter, depthMax, paths);  // pathtrace.cu:544
    for (int depth = 0; depth < depthMax; ++depth) {  // pathtrace.cu:561,597-602
      memset(isects.data(), 0, n * sizeof(ShadeableIntersection));  // pathtrace.cu:562
      runIntersect(depth, scene, nodes, paths, isects);              // pathtrace.cu:567
      for (int i = 0; i < n; ++i) {                                  // pathtrace.cu:584
        ref_blockIdx.x = (unsigned)i;
        shadeAndExtendRays(iter, depth, n, isects.data(), paths.data(), scene->materials.data(), (int)scene->materials.size(), nullptr, 0);
      }
    }
    for (int i = 0; i < n; ++i) {  // pathtrace.cu:610
      ref_blockIdx.x = (unsigned)i;
      finalGather(n, image.data(), paths.data());
    }
    ref_blockIdx.x = 0;
  }
  return image;
}

static int modeImages(gold::File& f, char** scenes) {
  // scene, width, height, depth, first iteration, iterations
  const int cases[][6] = {{0, 96, 64, 8, 1, 8},  {0, 61, 37, 8, 1, 16}, {0, 48, 32, 1, 1, 4},        {0, 48, 32, 2, 1, 4},
                          {0, 48, 32, 5, 1, 4},  {0, 48, 32, 20, 1, 4}, {1, 48, 32, 4, 1, 8},        {2, 48, 32, 8, 1, 8},
                          {3, 48, 32, 8, 1, 8},  {0, 48, 32, 8, 4194300, 8}, {0, 48, 32, 8, 2147483600, 4}};
  gold::Section& list = f.add("images", 6);
  int k = 0;
  for (const auto& c : cases) {
    Scene* scene = loadScene(scenes[c[0]], c[1], c[2]);
    startViewer(scene);
    std::vector<glm::vec3> img = renderSum(scene, c[3], c[4], c[5]);
    for (int j = 0; j < 6; ++j) list.w.push_back((uint32_t)c[j]);
    char name[24];
    snprintf(name, sizeof name, "sum_%d", k++);
    gold::Section& s = f.add(name, 3);
    for (const glm::vec3& p : img) putVec(s.w, p);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 9) {
    fprintf(stderr, "usage: ref_kernels camera,generate,intersect,shade,images OUT ISECT.bin SHADE_SCENE CORNELL SPHERE TWISTED QUIRKS\n");
    return 2;
  }
  const std::string modes = std::string(",") + argv[1] + ",";
  auto has = [&](const char* m) { return modes.find(std::string(",") + m + ",") != std::string::npos; };
  gold::File f;
  int rc = 0;
  if (has("camera")) modeCamera(f, argv + 5, 4);
  if (has("generate")) rc |= modeGenerate(f, argv + 5);
  if (has("intersect")) rc |= modeIntersect(f, argv[3], argv + 5);
  if (has("shade")) rc |= modeShade(f, argv[4]);
  if (has("images")) rc |= modeImages(f, argv + 5);
  if (f.sec.empty() || rc) return rc ? rc : 2;
  return f.write(argv[2]) ? 0 : 1;
}
