// pt_shade.inc — shadeAndExtendRays (pathtrace.cu:336-437): decisions, bounce sampling, the unfused k_shade stage kernel.
// Included by pt_kernels.hip inside ptk::<arith>::(anonymous).
// ───────────────────────────── shade ───────────────────────────────────────
PT_DEV void local_frame(f3 n, f3& tangent, f3& bitangent) {  // pathtrace.cu:216-223
  const bool a = __builtin_fabsf(n.x) > __builtin_fabsf(n.y);
  tangent = normalize(a ? mk(n.z, 0.f, -n.x) : mk(0.f, -n.z, n.y));
  bitangent = cross(n, tangent);
}
PT_DEV f3 sky_factor(f3 dir) {  // pathtrace.cu:360-362: skyColor * 0.5f
  const float t = 0.5f * (dir.y + 1.0f);
  const float w = (1.0f - t) * 1.0f;
  return scl(mk(w + t * 0.5f, w + t * 0.7f, w + t * 1.0f), 0.5f);
}

struct ShadeIO {
  f3 o, d, c;
  bool alive;
};
// shadeAndExtendRays (pathtrace.cu:336-437) for a LIVE path, split in two so that the wave can
// publish its survivor count (one atomic) while the expensive direction sampling still runs:
//   shade_decide  everything that determines whether the path survives and its new throughput:
//                 miss / emitter / Russian roulette / specular-vs-diffuse choice / colour product.
//                 Consumes the RNG draws the reference consumes up to that point, in its order.
//   shade_bounce  the new ray of a surviving path (remaining draws, sin/cos/acos).
// A live path at depth d has exactly trace_depth - d bounces left, so remainingBounces is implied.
// On `alive == false` the path retires with colour s.c; for a miss the sky factor has been applied
// (trace_depth - depth) times, which is what the reference's repeated passes over dead paths do
// (pathtrace.cu:356-366, SURVEY.md §8a).
struct Bounce {
  uint32_t rng_x;   // minstd state after the draws consumed by shade_decide
  int kind;         // 0 none, 1 specular, 2 diffuse
  float roughness;
};
PT_DEV Bounce shade_decide(const ptd::Mat* __restrict__ mats, int trace_depth, int depth, uint32_t seed, float ht, int hmat,
                           ShadeIO& s) {  // seed = iter_hash(iteration, depth) ^ utilhash(global pixel index), pathtrace.cu:205
  Bounce bo;
  bo.kind = 0;
  bo.rng_x = 1u;
  bo.roughness = 0.f;
  s.alive = false;
  if (ht < 0.0f) {
    const f3 sky = sky_factor(s.d);
    for (int k = depth; k < trace_depth; ++k) s.c = mul(s.c, sky);
    return bo;
  }
  MinStd rng(seed);
  const ptd::Mat* m = mats + hmat;
  const f3 mcolor = mk(m->color[0], m->color[1], m->color[2]);
  if (m->emittance > 0.0f) {
    s.c = mul(s.c, scl(mcolor, m->emittance));
    return bo;
  }
  if (depth > 3) {  // Russian roulette
    const float q = __builtin_fmaxf(mcolor.x, __builtin_fmaxf(mcolor.y, mcolor.z));
    if (rng.u01() > q) return bo;
    if (kFast) s.c = scl(s.c, __builtin_amdgcn_rcpf(q));
    else ieee::div3(s.c.x, s.c.y, s.c.z, q);
  }
  const float reflectivity = m->reflective;
  bo.roughness = 1.0f - m->refractive;
  if (reflectivity > 0.0f && rng.u01() < reflectivity) {
    bo.kind = 1;
    s.c = mul(s.c, mk(m->spec[0], m->spec[1], m->spec[2]));
  } else {
    bo.kind = 2;
    s.c = mul(s.c, mcolor);
  }
  bo.rng_x = rng.x;
  // remainingBounces-- : the path survives unless this was its last allowed bounce (its new ray
  // would never be traced, so it is not computed)
  s.alive = (depth + 1) < trace_depth;
  return bo;
}
// Direction sampling of the fast and fma modes: the same draws and the same formulas, evaluated in float only.
//   The trigonometric arguments are taken in REVOLUTIONS — sin(2*pi*u) of the draw u itself, and the specular angle
//   roughness*u1*pi/2 = roughness*u1/4 revolutions — so no 2*pi*u is rounded to float first (the reference rounds it, then calls sinf);
//   diffuse: cos(theta) = sqrt(1 - u1) =: s and sin(theta) = sin(acos(s)) = sqrt(1 - s*s) (one FMA keeps 1 - s*s exact
//   to one rounding), so neither acos nor a sincos of theta is evaluated.
//   HW (fast): v_sin_f32 / v_cos_f32 take revolutions directly, v_sqrt_f32.
//   !HW (fma): IEEE square roots and ptmath::sincos_rev (float polynomials, <= 1.6 ulp: the accuracy class of the sinf / cosf the
//   reference runs on under nvcc, which documents 2 ulp); the specular evaluations only when the wave holds a specular lane.
//   Round 3: the fma mode used to share the exact mode's sampling (fdlibm acosf + three double-reduced sincos, 900 issue cycles a
//   group); it is held to the tolerance, not to bit-equality, and the tolerance does not see the difference (tests/test_gpu_arith.py).
// Origin of the new ray (pathtrace.cu:420, :433): the hit point pushed 0.001 along the normal, in the build's arithmetic.
PT_DEV f3 bounce_origin(f3 hn, f3 hp) {
  if (kFast || kFloatTrig) return madd(hn, 0.001f, hp);
  return add(hp, scl(hn, 0.001f));
}
// shade_bounce in two halves, so that a kernel can put other work between them (k_paths takes new paths there, whose first bounce
// then runs through the same sampling): bounce_axis — the new origin and the axis the direction is sampled around,
// f = specular ? reflect(d, n) : n, after which the hit record and the old direction are dead — and bounce_sample, the remaining
// draws and the trigonometry.  A perfect mirror keeps the reflected direction, which IS its axis.
struct BounceAxis {
  f3 o, f;
};
PT_DEV f3 bounce_reflect(f3 d, f3 hn) {  // reflect(): incident - 2*dot(incident, n)*n, in the build's arithmetic
  if (kFast || kFloatTrig) return madd(hn, -2.0f * dot(d, hn), d);
  return sub(d, scl(hn, 2.0f * dot(d, hn)));
}
PT_DEV BounceAxis bounce_axis(const Bounce& bo, f3 hn, f3 hp, f3 d) {
  const f3 refl = bounce_reflect(d, hn);
  return BounceAxis{bounce_origin(hn, hp), bo.kind == 1 ? refl : hn};
}
template <bool HW>
PT_DEV f3 bounce_sample_float(const Bounce& bo, f3 f) {
  MinStd rng(1u);
  rng.x = bo.rng_x;
  const bool spec = bo.kind == 1;
  const float r1 = rng.u01(), r2 = rng.u01(), r3 = rng.u01();
  const float rev = bo.roughness * r1 * 0.25f;
  const float ct = HW ? __builtin_amdgcn_sqrtf(1.0f - r1) : __builtin_sqrtf(1.0f - r1);
  const float st2 = __builtin_fmaxf(fma_(-ct, ct, 1.0f), 0.0f);
  const float st = HW ? __builtin_amdgcn_sqrtf(st2) : __builtin_sqrtf(st2);
  float sA = 0.0f, cA = 1.0f, c1, s2;
  if (HW) {
    sA = __builtin_amdgcn_sinf(rev), cA = __builtin_amdgcn_cosf(rev);
    c1 = __builtin_amdgcn_cosf(r2);
    s2 = __builtin_amdgcn_sinf(spec ? r3 : r2);
  } else {
    ptmath::sincos_rev(r2, &s2, &c1);
    if (ballot(spec)) {  // wave-uniform
      float s3, c3;
      ptmath::sincos_rev(rev, &sA, &cA);
      ptmath::sincos_rev(r3, &s3, &c3);
      s2 = spec ? s3 : s2;
    }
  }
  const float sX = spec ? sA : st;
  const float cX = spec ? cA : ct;
  const float x = sX * c1, z = sX * s2, y = cX;
  f3 tangent, bitangent;
  local_frame(f, tangent, bitangent);
  const f3 pert = normalize(madd(tangent, x, madd(f, y, scl(bitangent, z))));
  const bool perturb = !spec || bo.roughness > 0.0f;
  return perturb ? pert : f;
}
PT_DEV f3 bounce_sample(const Bounce& bo, f3 f) {
  if (kFast) return bounce_sample_float<true>(bo, f);
  if (kFloatTrig) return bounce_sample_float<false>(bo, f);
  // The specular branch (pathtrace.cu:402-422) and the diffuse branch (:424-435, :225-238) have the
  // same shape — a frame around an axis f, three trigonometric evaluations, normalize(t*x + f*y + b*z)
  // — so both are evaluated by ONE instruction stream with per-lane operands instead of two divergent
  // branches executed back to back (a wave almost always holds both kinds).  Operations and their
  // order per lane are exactly the reference's:
  //   specular: f = reflect(d, n); angle = float(roughness*u1 * M_PI * 0.5f) [double product];
  //             x = float(sin(angle) * cos(2.0f*M_PI*u2)) [double], y = cos(angle),
  //             z = float(sin(angle) * sin(2.0f*M_PI*u3)) [double]
  //   diffuse:  f = n; theta = acos(sqrt(1-u1)); phi = float(2.0f*M_PI*u2) [double product];
  //             x = sin(theta)*cos(phi), y = cos(theta), z = sin(theta)*sin(phi)   [float]
  const double kPi = 3.14159265358979323846;
  MinStd rng(1u);
  rng.x = bo.rng_x;
  const bool spec = bo.kind == 1;
  const float r1 = rng.u01(), r2 = rng.u01(), r3 = rng.u01();  // diffuse consumes only two; the engine dies here
  const float angle = (float)((double)(bo.roughness * r1) * kPi * (double)0.5f);
  const float theta = ptmath::acosf32(__builtin_sqrtf(1.0f - r1));
  const float phi = (float)((double)2.0f * kPi * (double)r2);
  const float X = spec ? angle : theta;
  const double Y1 = spec ? (double)2.0f * kPi * (double)r2 : (double)phi;
  const double Y2 = spec ? (double)2.0f * kPi * (double)r3 : (double)phi;
  float sX, cX;
  ptmath::sincosf32(X, &sX, &cX);
  const float c1 = ptmath::cos_r(Y1);
  const float s2 = ptmath::sin_r(Y2);
  // specular: float(double(sX) * double(c1)) — the double product of two floats is exact, so it rounds
  // to the same value as the float product the diffuse branch forms
  const float x = sX * c1;
  const float z = sX * s2;
  const float y = cX;
  f3 tangent, bitangent;
  local_frame(f, tangent, bitangent);
  const f3 pert = normalize(add(add(scl(tangent, x), scl(f, y)), scl(bitangent, z)));
  const bool perturb = !spec || bo.roughness > 0.0f;  // a perfect mirror keeps the reflected direction: its axis
  return perturb ? pert : f;
}
PT_DEV void shade_bounce(const Bounce& bo, f3 hn, f3 hp, ShadeIO& s) {  // the two halves back to back
  const BounceAxis a = bounce_axis(bo, hn, hp, s.d);
  s.o = a.o;
  s.d = bounce_sample(bo, a.f);
}


__global__ __launch_bounds__(kBlock) void k_shade(SceneTables sc, BatchInfo b, int depth, ptd::Queues qs,
                                                  const int32_t* __restrict__ cnt_in, int32_t* __restrict__ cnt_out,
                                                  ptd::PathBuf in, ptd::HitBuf hits, ptd::PathBuf out,
                                                  ptd::RetireBuf ret) {
  extern __shared__ float4 lds_raw[];
  char* lds = reinterpret_cast<char*>(lds_raw);
  const ShadeLds L = shade_lds<true>(sc);
  stage16(lds + L.mats, sc.mats, mat_bytes(sc));
  uint32_t* ihash = reinterpret_cast<uint32_t*>(lds + L.ihash);
  iter_hash_fill(ihash, sc, b, depth);
  __syncthreads();
  const ptd::Mat* mats = reinterpret_cast<const ptd::Mat*>(lds + L.mats);

  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int lane = lane_id();
  const auto [q, r, wq] = wave_slot(wave, qs.Q, qs.W);
  const Retire rt = retire_of(ret, q);
  const int n_q = cnt_in[cnt_index(qs, 0, q)];
  const int64_t HS = hits.stride;
  const int64_t qbase = (int64_t)q * qs.cap;
  // inputs of one path; the next group's are loaded (branch-free, index clamped into the queue's own
  // region) while the current group is shaded
  struct In {
    PathTag tag;
    int hmat;
    float ht;
    f3 hn, hp, d, c;
  };
  const int last = qs.cap - 64 + lane;
  auto load = [&](int i) {
    In v;
    const int64_t at = qbase + min(i, last);
    v.ht = hits.t[at];
    v.hn = mk(hits.n[at], hits.n[HS + at], hits.n[2 * HS + at]);
    v.hmat = hits.mat[at];
    v.hp = mk(hits.p[at], hits.p[HS + at], hits.p[2 * HS + at]);
    path_load_tail(in, at, v.d, v.c, v.tag);
    return v;
  };
  In nx = load(r * 64 + lane);
  for (int j = r; j * 64 < n_q; j += wq) {
    const int i = j * 64 + lane;
    const bool valid = i < n_q;
    const In cur = nx;
    nx = load((j + wq) * 64 + lane);
    ShadeIO s;
    s.o = mk(0.f, 0.f, 0.f);
    s.d = cur.d;
    s.c = cur.c;
    s.alive = false;
    Bounce bo;
    bo.kind = 0;
    int k, pl;
    sample_of(cur.tag, b, k, pl);
    if (valid) bo = shade_decide(mats, b.trace_depth, depth, path_seed(k, pl, ihash, sc, b, depth), cur.ht, cur.hmat, s);
    // dead lanes: one record each at the front of region (q, k); survivors: ballot + popcount, ONE atomic per wave on the
    // queue's counter of the next depth, compacted stores
    retire_append(rt, valid && !s.alive, k, pl, s.c);
    const bool alive = valid && s.alive;
    const unsigned long long live = ballot(alive);
    int base = 0;
    if (live && lane == 0) base = atomicAdd(&cnt_out[cnt_index(qs, 0, q)], (int)__popcll(live));
    if (alive) shade_bounce(bo, cur.hn, cur.hp, s);
    if (live) {
      base = __builtin_amdgcn_readfirstlane(base);
      if (alive) path_store(out, qbase + base + rank_in(live), s.o, s.d, s.c, cur.tag);
    }
  }
}
