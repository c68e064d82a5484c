// oracle/ref_pt_harness.cpp — TEST INFRASTRUCTURE ONLY (golden generation).
//
// Pins what lives in src/pathtrace.cu and DOES compile with plain g++ to the reference's OWN code:
//   * buildBVH / buildBVHRecursive / computeBounds   src/pathtrace.cu:34-111  (host code; std::sort tie order included)
//   * intersectAABB                                  src/pathtrace.cu:113-128
//   * createLocalCoordinateSystem, sampleCosineWeightedHemisphere, reflect   src/pathtrace.cu:216-242
// pathtrace.cu as a whole cannot be compiled here (kernel-launch syntax, <cuda.h>, CUDA Thrust), but these functions are
// ordinary C++ between its kernels: the Makefile cuts the two line ranges 23-128 and 208-242 out of the file AT BUILD TIME
// into a scratch directory under /tmp (never into this repository, never onto the GPU box) and this harness includes them
// from there, next to the reference's own headers.  Under g++ the genuine NVIDIA host_defines.h (through sceneStructs.h's
// #include <cuda_runtime.h>, found inside the triton wheel) turns `__device__` into an ignored attribute, exactly as it
// does for intersections.h in ref_hot_harness.cpp.  Nothing of the reference is copied into the repository; the fixtures
// hold numbers only.
//
// The __global__ bodies (generateRayFromCamera, computeIntersections, shadeAndExtendRays, finalGather) and main.cpp's camera
// fix-up need stand-ins for the CUDA toolchain to compile; ref_kernels_harness.cpp holds those and pins them the same way.
// What still rests on SURVEY §4's KATs after both: the launch order of pathtrace()'s host loop, restated in that harness, and
// the mouse callbacks' double-precision increments, which pt_scene_orbit replaces by a float rule of its own.
//
// Modes:
//   ref_pt bvh     OUT.bin SCENE.txt...          per scene: the node table buildBVH returns (bounds, left, right, geomIndex)
//   ref_pt aabb    OUT.bin ISECT.bin SCENE.txt...  per scene: intersectAABB of every golden ray of ISECT.bin (the rays
//                                                ref_hot generated for the same scene list) against every node's box
//   ref_pt helpers OUT.bin                       the three sampling helpers on a grid of (u1, u2, normal / incident)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using std::max;  // CUDA's global min()/max() overloads exist only under nvcc (intersections.h:131,134)
using std::min;

#include "sceneStructs.h"
#include "scene.h"
#include "glm/glm.hpp"
#include "glm/gtx/norm.hpp"
#include "intersections.h"

#include "ref_pt_bvh.inc"      // src/pathtrace.cu:23-128, cut out at build time (oracle/Makefile)
#include "ref_pt_helpers.inc"  // src/pathtrace.cu:208-242

#include "ref_gold_io.h"

using gold::bitsf;
using gold::fbits;

static void putVec(std::vector<uint32_t>& w, const glm::vec3& v) {
  w.push_back(fbits(v.x));
  w.push_back(fbits(v.y));
  w.push_back(fbits(v.z));
}

static int modeBvh(const char* out, int nscenes, char** paths) {
  gold::File f;
  gold::Section& sets = f.add("sets", 2);  // per scene: geoms, nodes
  for (int s = 0; s < nscenes; ++s) {
    Scene* scene = new Scene(paths[s]);  // never deleted (scene.h:21 declares a destructor scene.cpp never defines)
    std::vector<BVHNodeGPU> nodes;
    buildBVH(scene->geoms, nodes);
    sets.w.push_back((uint32_t)scene->geoms.size());
    sets.w.push_back((uint32_t)nodes.size());
    char name[24];
    snprintf(name, sizeof name, "nodes_%d", s);  // bounds.min, bounds.max, left, right, geomIndex
    gold::Section& ns = f.add(name, 9);
    for (const BVHNodeGPU& n : nodes) {
      putVec(ns.w, n.bounds.min), putVec(ns.w, n.bounds.max);
      ns.w.push_back((uint32_t)n.left), ns.w.push_back((uint32_t)n.right), ns.w.push_back((uint32_t)n.geomIndex);
    }
  }
  return f.write(out) ? 0 : 1;
}

static int modeAabb(const char* out, const char* isect, int nscenes, char** paths) {
  gold::File in, f;
  if (!in.read(isect)) return 1;
  gold::Section& sets = f.add("sets", 3);  // per scene: nodes, rays, words per ray
  for (int s = 0; s < nscenes; ++s) {
    Scene* scene = new Scene(paths[s]);
    std::vector<BVHNodeGPU> nodes;
    buildBVH(scene->geoms, nodes);
    char name[24];
    snprintf(name, sizeof name, "rays_%d", s);
    const gold::Section* rs = in.find(name);
    if (!rs || rs->cols != 6) return 1;
    const uint32_t words = ((uint32_t)nodes.size() + 31u) / 32u;
    sets.w.push_back((uint32_t)nodes.size()), sets.w.push_back(rs->rows), sets.w.push_back(words);
    snprintf(name, sizeof name, "pass_%d", s);  // row = ray; bit n of the row = intersectAABB(nodes[n].bounds, ray)
    gold::Section& ps = f.add(name, words);
    for (uint32_t r = 0; r < rs->rows; ++r) {
      Ray ray;
      const uint32_t* w = rs->w.data() + 6 * (size_t)r;
      ray.origin = glm::vec3(bitsf(w[0]), bitsf(w[1]), bitsf(w[2]));
      ray.direction = glm::vec3(bitsf(w[3]), bitsf(w[4]), bitsf(w[5]));
      std::vector<uint32_t> row(words, 0u);
      for (size_t n = 0; n < nodes.size(); ++n)
        if (intersectAABB(nodes[n].bounds, ray)) row[n / 32] |= 1u << (n % 32);
      ps.w.insert(ps.w.end(), row.begin(), row.end());
    }
  }
  return f.write(out) ? 0 : 1;
}

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

static int modeHelpers(const char* out) {
  gold::File f;
  Rng rng(0x2545f491u);
  // normals: the six axis directions (the |x| > |y| branch of createLocalCoordinateSystem both ways and its tie x == y == 0),
  // diagonals with |x| == |y|, and random unit vectors
  std::vector<glm::vec3> normals = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
  normals.push_back(glm::normalize(glm::vec3(1.0f, 1.0f, 0.0f)));
  normals.push_back(glm::normalize(glm::vec3(-1.0f, 1.0f, 1.0f)));
  normals.push_back(glm::normalize(glm::vec3(1.0f, -1.0f, -2.0f)));
  while (normals.size() < 40) normals.push_back(rng.unit());
  // draws: the ends of [0, 1] (u01 can round up to exactly 1.0), values next to them, a lattice, random ones
  std::vector<float> us = {0.0f, 1.0f, 4.656612873077392578125e-10f, 0.99999994f, 0.25f, 0.5f, 0.75f, 0.3f, 0.7f, 0.125f};
  while (us.size() < 24) us.push_back(rng.u());
  {
    gold::Section& in = f.add("frame_in", 3);
    gold::Section& ou = f.add("frame_out", 6);  // tangent, bitangent
    for (const glm::vec3& n : normals) {
      glm::vec3 t(0.0f), b(0.0f);
      createLocalCoordinateSystem(n, t, b);
      putVec(in.w, n);
      putVec(ou.w, t), putVec(ou.w, b);
    }
  }
  {
    gold::Section& in = f.add("cosine_in", 5);  // u1, u2, normal
    gold::Section& ou = f.add("cosine_out", 3);
    for (const glm::vec3& n : normals)
      for (size_t i = 0; i < us.size(); ++i)
        for (size_t j = 0; j < us.size(); j += (i < 10 ? 1 : 5)) {
          const float u1 = us[i], u2 = us[j];
          const glm::vec3 v = sampleCosineWeightedHemisphere(u1, u2, n);
          in.w.push_back(fbits(u1)), in.w.push_back(fbits(u2));
          putVec(in.w, n);
          putVec(ou.w, v);
        }
  }
  {
    gold::Section& in = f.add("reflect_in", 6);  // incident, normal
    gold::Section& ou = f.add("reflect_out", 3);
    for (const glm::vec3& n : normals)
      for (int k = 0; k < 12; ++k) {
        glm::vec3 d = rng.unit();
        if (k == 0) d = -n;                       // head-on
        if (k == 1) d = glm::vec3(n.y, n.z, n.x);  // some fixed other direction
        const glm::vec3 v = reflect(d, n);
        putVec(in.w, d), putVec(in.w, n);
        putVec(ou.w, v);
      }
  }
  return f.write(out) ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "bvh")) return modeBvh(argv[2], argc - 3, argv + 3);
  if (argc >= 5 && !strcmp(argv[1], "aabb")) return modeAabb(argv[2], argv[3], argc - 4, argv + 4);
  if (argc == 3 && !strcmp(argv[1], "helpers")) return modeHelpers(argv[2]);
  fprintf(stderr, "usage: ref_pt bvh OUT SCENE... | aabb OUT ISECT.bin SCENE... | helpers OUT\n");
  return 2;
}
