// pt_arith.inc — float helpers and the primitive tests, included TWICE by pt_kernels.hip:
//   namespace ex   under `#pragma clang fp contract(off)`, neither fast nor fused: the reference's arithmetic
//                  (GLM operation order, IEEE divide / sqrt, no FMA) in EVERY build — used for the primary rays;
//   namespace md   under the build's own contraction setting in the build's mode: exact / fma / fast.
// The including file defines kFastArith (this namespace has the fast build's arithmetic) and kFusedRef (the fma build's
// explicit contractions, below) in the enclosing namespace first.
PT_DEV f3 add(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
PT_DEV f3 sub(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
PT_DEV f3 mul(f3 a, f3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
PT_DEV f3 scl(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
PT_DEV f3 neg(f3 a) { return mk(-a.x, -a.y, -a.z); }
// Scalar primitives of the arithmetic modes.  exact / fma: IEEE divide and square root (the compiler's correctly
// rounded expansions); fast: the hardware approximations v_rcp_f32 / v_rsq_f32 / v_sqrt_f32 (1 ulp).
PT_DEV float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
// (ieee::*: the same correctly rounded results as `/` and __builtin_sqrtf from a shorter instruction sequence, pt_kernels.hip)
PT_DEV float rcp_(float x) { return kFastArith ? __builtin_amdgcn_rcpf(x) : ieee::rcp(x); }
PT_DEV float div_(float a, float b) { return kFastArith ? a * __builtin_amdgcn_rcpf(b) : ieee::div(a, b); }
PT_DEV float sqrt_(float x) { return kFastArith ? __builtin_amdgcn_sqrtf(x) : ieee::sqrt(x); }
// kFusedRef (the fma build): sums of two products are contracted EXPLICITLY, first product fused, in the reference's
// association.  Left to the compiler, `a * b + c * d` becomes fma(a, b, c * d) or fma(c, d, a * b) depending on how many uses
// each product has after inlining — the same source then rounds differently in two kernels (seen: 1 ulp in the normalised
// bounce direction of 1 sample in 20,000 between k_paths and k_bounce, visible through the sky factor), and "one mode, one
// image" (tests/test_gpu_arith.py) is lost.  The forms below are the ones the compiler picks in the common case.
PT_DEV float dot(f3 a, f3 b) {
  if (kFastArith) return fma_(a.x, b.x, fma_(a.y, b.y, a.z * b.z));
  if (kFusedRef) return fma_(a.z, b.z, fma_(a.x, b.x, a.y * b.y));
  return (a.x * b.x + a.y * b.y) + a.z * b.z;
}
PT_DEV f3 cross(f3 x, f3 y) {
  if (kFusedRef || kFastArith) return mk(fma_(x.y, y.z, -(y.y * x.z)), fma_(x.z, y.x, -(y.z * x.x)), fma_(x.x, y.y, -(y.x * x.y)));
  return mk(x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y);
}
PT_DEV f3 normalize(f3 v) { return scl(v, kFastArith ? __builtin_amdgcn_rsqf(dot(v, v)) : ieee::rcp_sqrt(dot(v, v))); }
PT_DEV float length(f3 v) { return sqrt_(dot(v, v)); }
PT_DEV f3 madd(f3 a, float s, f3 b) {  // a * s + b
  if (kFastArith) return mk(fma_(a.x, s, b.x), fma_(a.y, s, b.y), fma_(a.z, s, b.z));
  return add(scl(a, s), b);
}

// vec3(m * vec4(v, w)) in GLM order: (m0*v0 + m1*v1) + (m2*v2 + m3*w); m is [c*3+r].  W is 0 (direction) or 1
// (point); fast: one multiply + FMA chain per row.
template <int W>
PT_DEV f3 mulMV(const float* m, f3 v) {
  f3 r;
  if (kFastArith) {
    r.x = fma_(m[0], v.x, fma_(m[3], v.y, W ? fma_(m[6], v.z, m[9]) : m[6] * v.z));
    r.y = fma_(m[1], v.x, fma_(m[4], v.y, W ? fma_(m[7], v.z, m[10]) : m[7] * v.z));
    r.z = fma_(m[2], v.x, fma_(m[5], v.y, W ? fma_(m[8], v.z, m[11]) : m[8] * v.z));
    return r;
  }
  const float w = (float)W;
  if (kFusedRef) {
    r.x = fma_(m[0], v.x, m[3] * v.y) + fma_(m[6], v.z, m[9] * w);
    r.y = fma_(m[1], v.x, m[4] * v.y) + fma_(m[7], v.z, m[10] * w);
    r.z = fma_(m[2], v.x, m[5] * v.y) + fma_(m[8], v.z, m[11] * w);
    return r;
  }
  r.x = (m[0] * v.x + m[3] * v.y) + (m[6] * v.z + m[9] * w);
  r.y = (m[1] * v.x + m[4] * v.y) + (m[7] * v.z + m[10] * w);
  r.z = (m[2] * v.x + m[5] * v.y) + (m[8] * v.z + m[11] * w);
  return r;
}


// Primitive tests.  The object-space transform of the ray and the world-space reconstruction of
// point / normal / distance are common to both types; only the middle (slab vs quadratic) differs.
// TYPE: 1 cube (boxIntersectionTest, intersections.h:48-90), 0 sphere (sphereIntersectionTest,
// intersections.h:102-144), -1 decided per lane from G->type.  Returns t (-1 = no hit).
// QO: the object-space origin is supplied by the caller (primary rays share the camera position, so it is one
// value per geom: computed once per block by the primary kernel, in the same operation order).
// (m * vec4(v, 1)) in the reference's operation order WITHOUT contraction, whatever the build's setting: the one
// ill-conditioned product of the primitive test (a thin wall's object-space coordinate is 100 * z + 500).  Rounding it like the
// reference removes 90 % of the remaining fma / fast sample flips (cornell 256^2 x 16 spp: 25 -> 3 pixels for fma, 46 -> 3 for
// fast; LABNOTES.md §3).
PT_DEV f3 mulMV_point_ref(const float* m, f3 v) {
#pragma clang fp contract(off)
  f3 r;
  r.x = (m[0] * v.x + m[3] * v.y) + (m[6] * v.z + m[9]);
  r.y = (m[1] * v.x + m[4] * v.y) + (m[7] * v.z + m[10]);
  r.z = (m[2] * v.x + m[5] * v.y) + (m[8] * v.z + m[11]);
  return r;
}

// Mesh extension: glm::intersectRayTriangle (external/include/glm/gtx/intersect.inl:37-74 of the reference's vendored GLM
// 0.9.6: Moeller-Trumbore, front faces only) on the world-space vertices kept in G->inv[0..8]; point / normal / returned
// distance in the conventions of the other two tests.  Operation order = oracle/pt_oracle.cpp triangleIntersectionTest.
PT_DEV float tri_test(const ptd::Geom* __restrict__ G, f3 ro, f3 rd, f3& point, f3& normal) {
  const f3 v0 = mk(G->inv[0], G->inv[1], G->inv[2]);
  const f3 e1 = sub(mk(G->inv[3], G->inv[4], G->inv[5]), v0);
  const f3 e2 = sub(mk(G->inv[6], G->inv[7], G->inv[8]), v0);
  const f3 p = cross(rd, e2);
  const float a = dot(e1, p);
  if (a < FLT_EPSILON) return -1.0f;
  const float f = rcp_(a);
  const f3 s = sub(ro, v0);
  const float bx = f * dot(s, p);
  if (bx < 0.0f || bx > 1.0f) return -1.0f;
  const f3 q = cross(s, e1);
  const float by = f * dot(rd, q);
  if (by < 0.0f || by + bx > 1.0f) return -1.0f;
  const float t = f * dot(e2, q);
  if (!(t >= 0.0f)) return -1.0f;
  point = kFastArith ? madd(rd, t - .0001f, ro) : add(ro, scl(normalize(rd), t - .0001f));  // getPointOnRay
  normal = normalize(cross(e1, e2));
  return length(sub(ro, point));
}

// DEFER: the world-space normal is left to finish_normal() (only a ray's winning candidate needs one): `normal` returns
// what that needs — the cube's object-space normal code, the sphere's object-space normal, times 4 where the hit is seen from
// inside (|normal| = 0.5, so its length tells; exact both ways, and a zero keeps its sign), a triangle's final normal.  (The
// flip itself waits for the finished normal, as in the reference: negating the INPUT negates every product but not a component
// whose terms cancel — +0 + -0 and -0 + +0 are both +0 — where the reference reports -0; tests/test_gpu_grid_rays.py, rays in
// a symmetry plane of a sphere.)
// rt_type >= 0: the primitive type when the caller already has it (TYPE < 0), which spares the read of G->type.
template <int TYPE, bool QO = false, bool DEFER = false>
PT_DEV float geom_test(const ptd::Geom* __restrict__ G_in, f3 ro_w, f3 rd_w, f3& point, f3& normal, f3 qo_pre = f3{0.f, 0.f, 0.f},
                       int rt_type = -1) {
  // records are 272 = 17 x 16 bytes in tables that start 16-byte aligned (LDS and memory alike): lets the matrix rows be read as
  // 16-byte words (ds_read_b128) instead of pairs of dwords
  const ptd::Geom* __restrict__ G = static_cast<const ptd::Geom*>(__builtin_assume_aligned(G_in, 16));
  const int gtype = TYPE >= 0 ? TYPE : (rt_type >= 0 ? rt_type : G->type);
  if (TYPE < 0 && gtype == 2) return tri_test(G, ro_w, rd_w, point, normal);  // mesh extension; never taken without meshes
  float inv[12];  // the inverse transform's three rows as three 16-byte reads
  {
    const v4f* gv = reinterpret_cast<const v4f*>(G->inv);
    const v4f r0 = gv[0], r1 = gv[1], r2 = gv[2];
    inv[0] = r0.x, inv[1] = r0.y, inv[2] = r0.z, inv[3] = r0.w, inv[4] = r1.x, inv[5] = r1.y, inv[6] = r1.z, inv[7] = r1.w;
    inv[8] = r2.x, inv[9] = r2.y, inv[10] = r2.z, inv[11] = r2.w;
  }
  const f3 qo = QO ? qo_pre : mulMV_point_ref(inv, ro_w);
  const f3 qd = normalize(mulMV<0>(inv, rd_w));
  const bool is_box = gtype == 1;
  float t;
  f3 nobj = mk(0.f, 0.f, 0.f);
  bool flip = false;
  int ncode = 0;  // cube: which of the 7 possible object-space normals (0 = zero vector, 1 + 2*axis + (sign > 0))
  if (is_box && kFastArith) {
    // fast mode: the unit cube is symmetric about the object-space origin, so with r = 1 / d, n = o * r and h = |r| / 2 the
    // near and far plane distances of an axis are -n - h and h - n: no min / max per axis, and the object-space normal's sign
    // is the sign of r (t2 < t1 iff r < 0).  The reference's scan over the axes (intersections.h:60-79) keeps the LARGEST
    // POSITIVE near distance (first axis on ties: strict >) and the SMALLEST far distance (first axis on ties: strict <):
    // a max3 / min3 and two compares each instead of the compare-and-select chain (half-rate instructions: -30 per candidate).
    // (reciprocals clamped to +-1e20: an axis the ray runs parallel to then gives huge finite distances of the right signs —
    // "never leaves the slab" inside it, "behind the ray" outside — instead of inf - inf)
    const float rx = __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(qd.x), -1e20f, 1e20f), ry = __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(qd.y), -1e20f, 1e20f),
                rz = __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(qd.z), -1e20f, 1e20f);
    const float nx = qo.x * rx, ny = qo.y * ry, nz = qo.z * rz;
    const float hx = __builtin_fabsf(rx) * 0.5f, hy = __builtin_fabsf(ry) * 0.5f, hz = __builtin_fabsf(rz) * 0.5f;
    const float tax = -nx - hx, tay = -ny - hy, taz = -nz - hz;
    const float tbx = hx - nx, tby = hy - ny, tbz = hz - nz;
    const float tnear = __builtin_fmaxf(__builtin_fmaxf(tax, tay), taz);  // v_max3_f32
    const float tfar = __builtin_fminf(__builtin_fminf(tbx, tby), tbz);
    const int cx = 1 + (int)(__float_as_uint(rx) >> 31), cy = 3 + (int)(__float_as_uint(ry) >> 31), cz = 5 + (int)(__float_as_uint(rz) >> 31);
    const bool outside = tnear > 0.f;  // some near plane lies ahead: the largest of them is the entry
    if (!(tfar > 0.f && (!outside || tfar >= tnear))) return -1.0f;
    const int cnear = tax == tnear ? cx : (tay == tnear ? cy : cz);
    const int cfar = tbx == tfar ? cx : (tby == tfar ? cy : cz);
    t = outside ? tnear : tfar;
    ncode = outside ? cnear : cfar;
  } else if (is_box) {
    float tmin = -1e38f, tmax = 1e38f;
    int tmin_c = 0, tmax_c = 0;
    const float qdv[3] = {qd.x, qd.y, qd.z};
    const float qov[3] = {qo.x, qo.y, qo.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float t1, t2;
      ieee::div2(-0.5f - qov[a], +0.5f - qov[a], qdv[a], t1, t2);
      const float ta = t1 < t2 ? t1 : t2;  // glm::min
      const float tb = t1 > t2 ? t1 : t2;  // glm::max
      const int c = 1 + 2 * a + (t2 < t1 ? 1 : 0);  // n[xyz] = t2 < t1 ? +1 : -1
      if (ta > 0.f && ta > tmin) {
        tmin = ta;
        tmin_c = c;
      }
      if (tb < tmax) {
        tmax = tb;
        tmax_c = c;
      }
    }
    if (!(tmax >= tmin && tmax > 0.f)) return -1.0f;
    if (tmin <= 0.f) {
      tmin = tmax;
      tmin_c = tmax_c;
    }
    t = tmin;
    ncode = tmin_c;
  } else {
    // radius .5 → powf(.5, 2) = .25
    const float along = dot(qo, qd);
    const float disc = kFastArith ? fma_(along, along, 0.25f - dot(qo, qo)) : along * along - (dot(qo, qo) - 0.25f);
    if (disc < 0.f) return -1.0f;
    const float root = sqrt_(disc);
    const float t1 = -along + root;
    const float t2 = -along - root;
    if (t1 < 0.f && t2 < 0.f) return -1.0f;
    if (t1 > 0.f && t2 > 0.f) {
      t = t2 < t1 ? t2 : t1;  // min(t1, t2)
    } else {
      t = t1 < t2 ? t2 : t1;  // max(t1, t2)
      flip = true;            // !outside → normal negated
    }
  }
  // getPointOnRay (intersections.h:27-29): origin + (t - .0001f) * normalize(direction); qd is already a unit
  // vector, so the fast mode does not normalise it a second time
  const f3 objp = kFastArith ? madd(qd, t - .0001f, qo) : add(qo, scl(normalize(qd), t - .0001f));
  if (!is_box) nobj = objp;
  float xf[12];
  {
    const v4f* gv = reinterpret_cast<const v4f*>(G->xf);
    const v4f r0 = gv[0], r1 = gv[1], r2 = gv[2];
    xf[0] = r0.x, xf[1] = r0.y, xf[2] = r0.z, xf[3] = r0.w, xf[4] = r1.x, xf[5] = r1.y, xf[6] = r1.z, xf[7] = r1.w;
    xf[8] = r2.x, xf[9] = r2.y, xf[10] = r2.z, xf[11] = r2.w;
  }
  // (the fast build could take the point as ro + rd * world distance and skip the `xf` fetch: C5 bounce kernel -5.3 %, but 0.27 %
  // of the random-scene pixels then move by > 1e-5, over tests/test_gpu_arith.py's bound of 0.2 %; LABNOTES.md §9.3)
  point = mulMV<1>(xf, objp);
  if (DEFER) {
    normal = is_box ? mk(__int_as_float(ncode), 0.f, 0.f) : (flip ? scl(nobj, 4.0f) : nobj);
  } else if (is_box) {
    normal = mk(G->box_normal[ncode][0], G->box_normal[ncode][1], G->box_normal[ncode][2]);  // precomputed, exact
  } else {
    normal = normalize(mulMV<0>(G->invT, nobj));
    if (flip) normal = neg(normal);
  }
  return length(sub(ro_w, point));
}
// The world-space normal of a hit whose geom_test ran with DEFER.
PT_DEV f3 finish_normal(const ptd::Geom* __restrict__ G, f3 stored) {
  const int gtype = G->type;
  if (gtype == 1) {
    const int c = __float_as_int(stored.x);
    return mk(G->box_normal[c][0], G->box_normal[c][1], G->box_normal[c][2]);
  }
  if (gtype == 2) return stored;
  const bool flip = dot(stored, stored) > 1.0f;  // 0.25 outside, 4 inside
  const f3 n = normalize(mulMV<0>(G->invT, flip ? scl(stored, 0.25f) : stored));
  return flip ? neg(n) : n;
}


// intersectAABB (pathtrace.cu:113-128) with the reciprocal direction hoisted (the reference
// recomputes 1/dir per node, same value) and the swap expressed as a select on its sign.
// The reference returns false at the first axis with tmax <= tmin; tmin only grows and tmax only
// shrinks, so one test after the third axis is equivalent.
// Reciprocal direction of a ray starting at o.  fast: |d| is clamped to >= 1e-20 so that the reciprocal stays finite
// (an axis-parallel ray would otherwise produce inf - inf in the FMA form of the slab test).
PT_DEV RayInv ray_inv(f3 d, f3 o) {
  RayInv r;
  if (kFastArith) {
    const float dx = __builtin_copysignf(__builtin_fmaxf(__builtin_fabsf(d.x), 1e-20f), d.x);
    const float dy = __builtin_copysignf(__builtin_fmaxf(__builtin_fabsf(d.y), 1e-20f), d.y);
    const float dz = __builtin_copysignf(__builtin_fmaxf(__builtin_fabsf(d.z), 1e-20f), d.z);
    r.ix = __builtin_amdgcn_rcpf(dx), r.iy = __builtin_amdgcn_rcpf(dy), r.iz = __builtin_amdgcn_rcpf(dz);
  } else {
    ieee::rcp3(d.x, d.y, d.z, r.ix, r.iy, r.iz);
  }
  r.sx = r.ix < 0.0f, r.sy = r.iy < 0.0f, r.sz = r.iz < 0.0f;
  r.nx = -o.x * r.ix, r.ny = -o.y * r.iy, r.nz = -o.z * r.iz;
  return r;
}
// Slab test from the six plane distances (near/far per axis by min/max): the fast-mode form.
PT_DEV bool slab_planes(float ax, float bx, float ay, float by, float az, float bz, float& tn) {
  const float t0 = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(ax, bx), __builtin_fminf(ay, by)), __builtin_fminf(az, bz));
  const float t1 = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(ax, bx), __builtin_fmaxf(ay, by)), __builtin_fmaxf(az, bz));
  tn = __builtin_fmaxf(t0, 0.0f);
  return !(t1 <= tn);
}
// slab() that also returns the entry distance (for the closer-hit cull of the subtree scans).
PT_DEV bool slab_t(f3 o, const RayInv& ri, float lox, float loy, float loz, float hix, float hiy, float hiz, float& tn) {
  if (kFastArith) {
    // The fast build's bounce kernels get their boxes as CENTRE (lo*) and HALF EXTENT (hi*) (SceneTables::*_b, converted by the
    // host): the plane distances of an axis are tc -+ h * |i| with tc = c * i - o * i — three FMAs per axis and no min / max
    // (min / max / compare / select issue at half the rate of an FMA on gfx950, profiles/r03_ubench_valu.txt: 41 instead
    // of 59 SIMD cycles per box).
    const float tcx = fma_(lox, ri.ix, ri.nx), tcy = fma_(loy, ri.iy, ri.ny), tcz = fma_(loz, ri.iz, ri.nz);
    const float ax = __builtin_fabsf(ri.ix), ay = __builtin_fabsf(ri.iy), az = __builtin_fabsf(ri.iz);
    const float t0 = __builtin_fmaxf(__builtin_fmaxf(fma_(-hix, ax, tcx), fma_(-hiy, ay, tcy)), fma_(-hiz, az, tcz));
    const float t1 = __builtin_fminf(__builtin_fminf(fma_(hix, ax, tcx), fma_(hiy, ay, tcy)), fma_(hiz, az, tcz));
    tn = __builtin_fmaxf(t0, 0.0f);
    return !(t1 <= tn);
  }
  const float t0x = ((ri.sx ? hix : lox) - o.x) * ri.ix;
  const float t1x = ((ri.sx ? lox : hix) - o.x) * ri.ix;
  const float t0y = ((ri.sy ? hiy : loy) - o.y) * ri.iy;
  const float t1y = ((ri.sy ? loy : hiy) - o.y) * ri.iy;
  const float t0z = ((ri.sz ? hiz : loz) - o.z) * ri.iz;
  const float t1z = ((ri.sz ? loz : hiz) - o.z) * ri.iz;
  const float tmin = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(0.0f, t0x), t0y), t0z);
  const float tmax = __builtin_fminf(__builtin_fminf(__builtin_fminf(FLT_MAX, t1x), t1y), t1z);
  tn = tmin;
  return !(tmax <= tmin);
}
PT_DEV bool slab(f3 o, const RayInv& ri, float lox, float loy, float loz, float hix, float hiy, float hiz) {
  float tn;
  return slab_t(o, ri, lox, loy, loz, hix, hiy, hiz, tn);
}
// slab() on a box given relative to the ray origin (lo - o, hi - o precomputed with the same subtraction).
PT_DEV bool slab_rel(const RayInv& ri, float lox, float loy, float loz, float hix, float hiy, float hiz) {
  if (kFastArith) {
    float tn;
    return slab_planes(lox * ri.ix, hix * ri.ix, loy * ri.iy, hiy * ri.iy, loz * ri.iz, hiz * ri.iz, tn);
  }
  const float t0x = (ri.sx ? hix : lox) * ri.ix;
  const float t1x = (ri.sx ? lox : hix) * ri.ix;
  const float t0y = (ri.sy ? hiy : loy) * ri.iy;
  const float t1y = (ri.sy ? loy : hiy) * ri.iy;
  const float t0z = (ri.sz ? hiz : loz) * ri.iz;
  const float t1z = (ri.sz ? loz : hiz) * ri.iz;
  const float tmin = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(0.0f, t0x), t0y), t0z);
  const float tmax = __builtin_fminf(__builtin_fminf(__builtin_fminf(FLT_MAX, t1x), t1y), t1z);
  return !(tmax <= tmin);
}


// generateRayFromCamera (pathtrace.cu:270-286) for global pixel index p:
// dir = normalize(view - right*pl.x*(x - W/2) - up*pl.y*(y - H/2)); no jitter, `iter` unused.
// aa: the stochastic anti-aliasing extension (PtOptions.aa_jitter; the reference has none): the sample position moves by
// (jx, jy) in [-0.5, 0.5] inside the pixel.  aa == false is the reference's expression, unchanged.
PT_DEV f3 camera_dir(const ptd::Camera& cam, float inv_w, int p, bool aa = false, float jx = 0.0f, float jy = 0.0f) {
  int x, y;
  divmod(p, cam.res_x, inv_w, y, x);
  const float fx = aa ? ((float)x + jx) - cam.res_x * 0.5f : (float)x - cam.res_x * 0.5f;
  const float fy = aa ? ((float)y + jy) - cam.res_y * 0.5f : (float)y - cam.res_y * 0.5f;
  const f3 view = mk(cam.view[0], cam.view[1], cam.view[2]);
  const f3 a = scl(scl(mk(cam.right[0], cam.right[1], cam.right[2]), cam.pl_x), fx);
  const f3 c = scl(scl(mk(cam.up[0], cam.up[1], cam.up[2]), cam.pl_y), fy);
  return normalize(sub(sub(view, a), c));
}

