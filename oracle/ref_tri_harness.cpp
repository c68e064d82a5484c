// oracle/ref_tri_harness.cpp — TEST INFRASTRUCTURE ONLY (golden generation).
//
// Pins the mesh extension's triangle test to the reference's OWN vendored code, compiled in place from /root/reference:
//   * external/include/glm/gtx/intersect.inl:37-74 (glm::intersectRayTriangle of GLM 0.9.6.3), through the unmodified
//     <glm/gtx/intersect.hpp>;
//   * src/intersections.h:27-29 (getPointOnRay), included unmodified — which needs the same <cuda_runtime.h> include path
//     as ref_hot_harness.cpp (sceneStructs.h:5) and the same two lines of glue for min / max.
// The reference has no triangle primitive of its own: what the extension adds around GLM's function — the point pulled
// back by getPointOnRay(r, bary.z), the normal normalize(cross(e1, e2)), the distance length(origin - point) — is the
// extension's convention (csrc/pt_arith.inc tri_test), restated below in four lines with the reference's getPointOnRay and
// GLM's functions.  GLM's decision and its baryPosition are the pinned part.
//
//   ref_tri OUT.bin      sections (format: ref_gold_io.h):
//     tris    [24, 9]      world-space vertices v0 v1 v2 of the fixed triangle set
//     sets    [1, 2]       24, 1024 (the layout tests/golden_io.py expected_closest_hits reads)
//     rays_0  [1024, 6]    origin, direction
//     rayinfo [1024, 3]    family (index into FAMILY below), target triangle, feature (edge i runs from vertex i to
//                          vertex (i + 1) % 3; vertex i; 0 where the aim is a face point)
//     bary    [24576, 4]   row = ray * 24 + triangle: GLM's return value, baryPosition.xyz (zeroed before each call)
//     hits_0  [24576, 8]   the column layout of ref_isect's hits_*: distance (-1 = miss), point, normal, 1 for a hit
// Inputs come from our own xorshift generator and use +, -, *, / and sqrt only, so the file is the same on every machine.
// Built by `make -C oracle ref` into oracle/_ref/ (git-ignored); never shipped; only the fixture travels.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
using std::max;  // CUDA's global min()/max() overloads exist only under nvcc; intersections.h calls them unqualified
using std::min;

#include "intersections.h"

#include "ref_gold_io.h"

using gold::fbits;

enum Family { FACE, EDGE, VERTEX, HAIR, BACK, GRAZING, ON_PLANE, AXIS, FAR, NFAMILIES };
static const int COUNT[NFAMILIES] = {160, 192, 96, 192, 96, 96, 96, 48, 48};  // 1024 rays
static const int NTRI = 24;

struct Rng {  // as ref_hot_harness.cpp
  uint32_t s;
  explicit Rng(uint32_t seed) : s(seed ? seed : 1u) {}
  uint32_t next() {
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return s;
  }
  double u() { return (double)(next() >> 8) * (1.0 / 16777216.0); }  // [0,1)
  double range(double a, double b) { return a + (b - a) * u(); }
};

struct D3 {
  double x, y, z;
};
static D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static D3 operator*(double s, D3 a) { return {s * a.x, s * a.y, s * a.z}; }
static double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static double len(D3 a) { return sqrt(dot(a, a)); }
static D3 unit(D3 a) { return (1.0 / len(a)) * a; }
static D3 d3(const glm::vec3& v) { return {(double)v.x, (double)v.y, (double)v.z}; }
static float f32nz(double v) {  // rounded, and never -0.0 (the scene loader may return +0 for it)
  float f = (float)v;
  return f == 0.0f ? 0.0f : f;
}
static glm::vec3 v3(D3 a) { return glm::vec3((float)a.x, (float)a.y, (float)a.z); }

struct Tri {
  glm::vec3 v[3];
};

static void addTri(std::vector<Tri>& t, D3 a, D3 b, D3 c) {
  Tri r;
  const D3 p[3] = {a, b, c};
  for (int i = 0; i < 3; ++i) r.v[i] = glm::vec3(f32nz(p[i].x), f32nz(p[i].y), f32nz(p[i].z));
  t.push_back(r);
}

static std::vector<Tri> makeTris() {
  std::vector<Tri> t;
  // 0-7: a closed octahedron, scaled by (1.5, 0.8, 1.1), rotated by the rational rotation (1/3)[2 -1 2; 2 2 -1; -1 2 2]
  // and moved to (0.3, 1, -0.5); outward faces counter-clockwise (the order of scenes._octahedron_tris)
  {
    const D3 c = {0.3, 1.0, -0.5}, sc = {1.5, 0.8, 1.1};
    auto xf = [&](D3 p) {
      D3 q = {sc.x * p.x, sc.y * p.y, sc.z * p.z};
      D3 r = {(2 * q.x - q.y + 2 * q.z) / 3.0, (2 * q.x + 2 * q.y - q.z) / 3.0, (-q.x + 2 * q.y + 2 * q.z) / 3.0};
      return c + r;
    };
    for (int sx = 1; sx >= -1; sx -= 2)
      for (int sy = 1; sy >= -1; sy -= 2)
        for (int sz = 1; sz >= -1; sz -= 2) {
          D3 a = {(double)sx, 0, 0}, b = {0, (double)sy, 0}, d = {0, 0, (double)sz};
          if (sx * sy * sz < 0) std::swap(b, d);
          addTri(t, xf(a), xf(b), xf(d));
        }
  }
  // 8-9: an axis-aligned quad in the plane z = -2 (a flat leaf box; zero coordinates), facing +z
  addTri(t, {0, 0, -2}, {2, 0, -2}, {2, 1.5, -2});
  addTri(t, {0, 0, -2}, {2, 1.5, -2}, {0, 1.5, -2});
  // 10-13: a fan of four around one vertex
  {
    const D3 apex = {-3, 2, 0.5}, rim[4] = {{-2, 2, 0}, {-3, 3, 0}, {-4, 2, 0}, {-3, 1, 0}};
    for (int i = 0; i < 4; ++i) addTri(t, apex, rim[i], rim[(i + 1) % 4]);
  }
  // 14-17: small right triangles with legs L: for a head-on unit direction a = dot(e1, cross(d, e2)) = L * L, from
  // 1.4e-7 to 3.6e-7, which the incidence (cosine 0.2 to 1) takes to either side of FLT_EPSILON = 1.19e-7
  {
    const double L[4] = {3.8e-4, 4.2e-4, 5e-4, 6e-4};
    for (int i = 0; i < 4; ++i) {
      D3 a = {1.5 + 0.1 * i, -1.5, 0.25};
      addTri(t, a, a + D3{L[i], 0, 0}, a + D3{0, L[i], 0});
    }
  }
  // 18-19: slivers, aspect 1000 : 1
  addTri(t, {-1, -2, 1}, {1, -2, 1}, {0.3, -1.998, 1.001});
  addTri(t, {3, 0, 1}, {3, 2, 1.5}, {3.002, 1, 1.25});
  // 20-21: large ones, edges of 100
  addTri(t, {-50, -6, 50}, {50, -6, 50}, {0, -6, -50});
  addTri(t, {-40, -8, -60}, {60, -9, -55}, {10, 40, -70});
  // 22-23: far from the origin
  addTri(t, {100, 101, 99}, {101.5, 100.2, 99.5}, {100.4, 102, 100.3});
  addTri(t, {-100, -98, 103}, {-99, -99.5, 101}, {-101, -97, 101.7});
  return t;
}

struct RayRec {
  Ray r;
  int family, target, feature;
};

// The condition on the `face` rays, in float64 on the float32 inputs: against EVERY triangle the decision of
// intersectRayTriangle is made with every comparison clear of its boundary — the barycentrics by 1e-3 of 1, the distance by
// 1e-3 of the origin's distance, a by 1e-2 of FLT_EPSILON — and each by no less than 32 float32 roundings of the terms that
// are summed (a small triangle seen from far away has a large 1 / a; a sliver's a is small against |e1||e2|).
static bool clearOfEveryBoundary(const std::vector<Tri>& tris, const Ray& r) {
  const D3 o = d3(r.origin), d = d3(r.direction);
  const double E = 32.0 * (double)FLT_EPSILON;
  for (const Tri& tr : tris) {
    const D3 v0 = d3(tr.v[0]), e1 = d3(tr.v[1]) - v0, e2 = d3(tr.v[2]) - v0;
    const D3 p = cross(d, e2);
    const double a = dot(e1, p);
    if (fabs(a - (double)FLT_EPSILON) < std::max(1e-2 * (double)FLT_EPSILON, E * len(e1) * len(e2))) return false;
    if (a < (double)FLT_EPSILON) continue;
    const double f = 1.0 / a;
    const D3 s = o - v0;
    const double bx = f * dot(s, p), mx = std::max(1e-3, E * f * len(s) * len(p));
    if (fabs(bx) < mx || fabs(bx - 1.0) < mx) return false;
    if (bx < 0.0 || bx > 1.0) continue;
    const D3 q = cross(s, e1);
    const double by = f * dot(d, q), my = std::max(1e-3, E * f * len(q)) + mx;
    if (fabs(by) < my || fabs(by + bx - 1.0) < my) return false;
    if (by < 0.0 || by + bx > 1.0) continue;
    const double t = f * dot(e2, q), mt = std::max(1e-3 * len(s), E * f * len(e2) * len(q));
    if (fabs(t) < mt) return false;
  }
  return true;
}

struct Maker {
  const std::vector<Tri>& tris;
  Rng rng;
  std::vector<RayRec> out;
  explicit Maker(const std::vector<Tri>& t) : tris(t), rng(0x7a11c0deu) {}

  D3 vert(int k, int i) const { return d3(tris[k].v[i]); }
  D3 normalOf(int k) const { return unit(cross(vert(k, 1) - vert(k, 0), vert(k, 2) - vert(k, 0))); }
  double sizeOf(int k) const {
    return std::min(len(vert(k, 1) - vert(k, 0)), std::min(len(vert(k, 2) - vert(k, 1)), len(vert(k, 0) - vert(k, 2))));
  }
  // origins of the families that look from nearby: 1 to 8 away, less for the small triangles
  double nearDist(int k) { return std::min(1.0, 20.0 * sizeOf(k)) * rng.range(1.0, 8.0); }
  void tangents(D3 n, D3& t1, D3& t2) const {
    D3 ax = fabs(n.x) <= fabs(n.y) && fabs(n.x) <= fabs(n.z) ? D3{1, 0, 0} : fabs(n.y) <= fabs(n.z) ? D3{0, 1, 0} : D3{0, 0, 1};
    t1 = unit(cross(n, ax));
    t2 = cross(n, t1);
  }
  D3 inPlaneUnit(int k) {  // a random unit vector in the triangle's plane
    D3 t1, t2;
    tangents(normalOf(k), t1, t2);
    for (;;) {
      double x = rng.range(-1, 1), y = rng.range(-1, 1), l2 = x * x + y * y;
      if (l2 > 1e-3 && l2 <= 1.0) return (1.0 / sqrt(l2)) * (x * t1 + y * t2);
    }
  }
  D3 toward(int k, double c) {  // unit vector whose component along the triangle's normal is c
    return c * normalOf(k) + sqrt(std::max(0.0, 1.0 - c * c)) * inPlaneUnit(k);
  }
  D3 facePoint(int k) {  // all three barycentrics >= 0.05
    double a = rng.u(), b = rng.u();
    if (a + b > 1.0) a = 1.0 - a, b = 1.0 - b;
    double w1 = 0.05 + 0.85 * a, w2 = 0.05 + 0.85 * b;
    return (1.0 - w1 - w2) * vert(k, 0) + w1 * vert(k, 1) + w2 * vert(k, 2);
  }
  D3 edgePoint(int k, int e) {
    double s = rng.range(0.02, 0.98);
    return (1.0 - s) * vert(k, e) + s * vert(k, (e + 1) % 3);
  }
  D3 inwardOfEdge(int k, int e) const {  // in the plane, perpendicular to edge e, towards the third vertex
    D3 a = vert(k, e), b = vert(k, (e + 1) % 3), c = vert(k, (e + 2) % 3);
    D3 ed = unit(b - a), w = c - a;
    return unit(w - dot(w, ed) * ed);
  }
  D3 aimOfKind(int kind, int k, int& feature) {  // 0 face, 1 edge, 2 vertex
    feature = kind ? (int)(rng.next() % 3u) : 0;
    return kind == 0 ? facePoint(k) : kind == 1 ? edgePoint(k, feature) : vert(k, feature);
  }
  void push(int fam, int k, int feature, D3 o, D3 d) {
    RayRec rr;
    rr.r.origin = v3(o);
    rr.r.direction = v3(d);
    rr.family = fam, rr.target = k, rr.feature = feature;
    out.push_back(rr);
  }
  // from the float32 origin towards q: normalised in float64, then rounded
  void aimed(int fam, int k, int feature, D3 q, D3 w, double dist) {
    glm::vec3 o32 = v3(q + dist * w);
    push(fam, k, feature, d3(o32), unit(q - d3(o32)));
  }

  bool make() {
    // face: every fourth ray from the back
    int tries = 0;
    for (int n = 0; n < COUNT[FACE]; ++tries) {
      if (tries > 200000) return false;
      int k = tries % NTRI;
      double c = rng.range(0.2, 1.0) * ((tries / NTRI) % 4 == 3 ? -1.0 : 1.0);
      aimed(FACE, k, 0, facePoint(k), toward(k, c), nearDist(k));
      if (clearOfEveryBoundary(tris, out.back().r)) ++n;
      else out.pop_back();
    }
    for (int n = 0; n < COUNT[EDGE]; ++n) {
      int k = n % NTRI, e = (n / NTRI) % 3;
      aimed(EDGE, k, e, edgePoint(k, e), toward(k, rng.range(0.2, 1.0)), nearDist(k));
    }
    for (int n = 0; n < COUNT[VERTEX]; ++n) {
      int k = n % NTRI, i = (n / NTRI) % 3;
      aimed(VERTEX, k, i, vert(k, i), toward(k, rng.range(0.2, 1.0)), nearDist(k));
    }
    {  // hair: the edge aim moved in the plane by +-{1e-8 ... 1e-5} of 1 + |p| (tests/grazing_rays.py DELTAS)
      const double mags[6] = {1e-8, 3e-8, 1e-7, 3e-7, 1e-6, 1e-5};
      for (int n = 0; n < COUNT[HAIR]; ++n) {
        int k = n % NTRI, e = (n / NTRI) % 3;
        double delta = mags[(n / 2) % 6] * (n % 2 ? -1.0 : 1.0);
        if ((n / NTRI) % 2) delta = mags[(n / 3) % 6] * ((n / 7) % 2 ? -1.0 : 1.0);
        D3 p = edgePoint(k, e);
        aimed(HAIR, k, e, p + (delta * (1.0 + len(p))) * inwardOfEdge(k, e), toward(k, rng.range(0.2, 1.0)), nearDist(k));
      }
    }
    for (int n = 0; n < COUNT[BACK]; ++n) {
      int k = n % NTRI, feature;
      D3 q = aimOfKind((n / NTRI) % 3, k, feature);
      aimed(BACK, k, feature, q, toward(k, -rng.range(0.2, 1.0)), nearDist(k));
    }
    {  // grazing: the direction within 1e-7 ... 1e-3 of the plane, from either side
      const double eps[6] = {1e-7, 1e-6, 1e-5, 1e-4, 3e-4, 1e-3};
      for (int n = 0; n < COUNT[GRAZING]; ++n) {
        int k = n % NTRI;
        double c = eps[(n / 2) % 6] * (n % 2 ? -1.0 : 1.0);
        aimed(GRAZING, k, 0, facePoint(k), toward(k, c), std::min(1.0, 20.0 * sizeOf(k)) * rng.range(1.0, 3.0));
      }
    }
    {  // on plane: origins within +-2e-4 of the plane, looking through it from the front side's direction
      const double hs[8] = {0.0, 1e-6, 1e-5, 5e-5, 9e-5, 1.1e-4, 1.5e-4, 2e-4};
      for (int n = 0; n < COUNT[ON_PLANE]; ++n) {
        int k = n % NTRI;
        double h = hs[(n / 2) % 8] * (n % 2 ? -1.0 : 1.0);
        D3 q = facePoint(k);
        push(ON_PLANE, k, 0, q + h * normalOf(k), -1.0 * toward(k, rng.range(0.2, 1.0)));
      }
    }
    for (int n = 0; n < COUNT[AXIS]; ++n) {  // axis-parallel directions with signed zeros: the quad and the octahedron
      int k = n % 10, feature, axis = (n / 2) % 3;
      D3 q = aimOfKind(n % 3, k, feature);
      double sgn = dot(normalOf(k), D3{axis == 0 ? 1.0 : 0.0, axis == 1 ? 1.0 : 0.0, axis == 2 ? 1.0 : 0.0}) >= 0 ? -1.0 : 1.0;
      if (n % 5 == 4) sgn = -sgn;  // some from behind
      D3 o = q, d = {0, 0, 0};
      double dist = rng.range(1.0, 8.0);
      (axis == 0 ? o.x : axis == 1 ? o.y : o.z) -= sgn * dist;
      (axis == 0 ? d.x : axis == 1 ? d.y : d.z) = sgn;
      push(AXIS, k, feature, d3(v3(o)), d);
      glm::vec3& dd = out.back().r.direction;
      uint32_t bitsz = rng.next();
      for (int c = 0; c < 3; ++c)
        if (c != axis && ((bitsz >> c) & 1u)) dd[c] = -0.0f;
    }
    for (int n = 0; n < COUNT[FAR]; ++n) {
      int k = n % NTRI, feature;
      D3 q = aimOfKind((n / NTRI + n) % 3, k, feature);
      aimed(FAR, k, feature, q, toward(k, rng.range(0.2, 1.0)), rng.range(100.0, 1000.0));
    }
    return out.size() == 1024;
  }
};

static void putVec(std::vector<uint32_t>& w, const glm::vec3& v) {
  w.push_back(fbits(v.x));
  w.push_back(fbits(v.y));
  w.push_back(fbits(v.z));
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: ref_tri OUT.bin\n");
    return 2;
  }
  const std::vector<Tri> tris = makeTris();
  if ((int)tris.size() != NTRI) return 1;
  Maker mk(tris);
  if (!mk.make()) {
    fprintf(stderr, "ref_tri: the face family could not be filled\n");
    return 1;
  }
  gold::File f;
  gold::Section& ts = f.add("tris", 9);
  for (const Tri& t : tris)
    for (int i = 0; i < 3; ++i) putVec(ts.w, t.v[i]);
  gold::Section& sets = f.add("sets", 2);
  sets.w.push_back((uint32_t)NTRI);
  sets.w.push_back((uint32_t)mk.out.size());
  gold::Section& rs = f.add("rays_0", 6);
  gold::Section& ri = f.add("rayinfo", 3);
  for (const RayRec& rr : mk.out) {
    putVec(rs.w, rr.r.origin), putVec(rs.w, rr.r.direction);
    ri.w.push_back((uint32_t)rr.family), ri.w.push_back((uint32_t)rr.target), ri.w.push_back((uint32_t)rr.feature);
  }
  gold::Section& bs = f.add("bary", 4);
  gold::Section& hs = f.add("hits_0", 8);
  for (const RayRec& rr : mk.out)
    for (const Tri& t : tris) {
      const Ray& r = rr.r;
      glm::vec3 bary(0.0f);
      const bool hit = glm::intersectRayTriangle(r.origin, r.direction, t.v[0], t.v[1], t.v[2], bary);
      bs.w.push_back(hit ? 1u : 0u);
      putVec(bs.w, bary);
      float dist = -1.0f;
      glm::vec3 p(0.0f), n(0.0f);
      if (hit) {  // the extension's convention around GLM's result (csrc/pt_arith.inc tri_test)
        p = getPointOnRay(r, bary.z);
        n = glm::normalize(glm::cross(t.v[1] - t.v[0], t.v[2] - t.v[0]));
        dist = glm::length(r.origin - p);
      }
      hs.w.push_back(fbits(dist));
      putVec(hs.w, p), putVec(hs.w, n);
      hs.w.push_back(hit ? 1u : 0u);
    }
  return f.write(argv[1]) ? 0 : 1;
}
