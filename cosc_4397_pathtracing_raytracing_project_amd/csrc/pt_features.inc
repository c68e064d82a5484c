// pt_features.inc — first-hit feature buffers (include/pt_amd.h, pt_render_features): per tile pixel the running sums of
// what the camera ray of every iteration sees — normal, hit distance, material colour, hit count, intersection point — and
// the object id of the last iteration.  Included by pt_kernels.hip inside ptk::<arith>::(anonymous), after the traversal code.
//
// The camera ray of sample (iteration, global pixel) is generated in registers exactly as k_generate / k_primary generate
// it (Ar<kD0>::camera_dir + aa_jitter) and its closest hit comes from the depth-0 machinery in the depth-0 arithmetic on the
// reference-arithmetic tables (sc.top / sc.nodes): the same hit records in the exact, fma and fast builds, bit for bit.
//   * one wave owns groups of 64 consecutive tile pixels (group g = pixels 64 g .. 64 g + 63; the tail group is masked);
//   * per group it loads the three float4 accumulators of its lanes once, loops over the call's iterations with the sums in
//     registers and stores them once: one 16-byte access per lane and plane, 1 KB contiguous per wave and plane — 96 B of
//     memory traffic per pixel and call whatever the iteration count, no atomics, no ray or hit record through HBM;
//   * every sum is a plain float add per iteration, in iteration order (a miss adds +0).  Without anti-aliasing every
//     iteration has the same ray: it is traced once and its values are added once per iteration — K adds, not one multiply.
// TABLES_IN_LDS / PACKET: where the tables live and how candidates are found, as for k_intersect and k_primary<kTopScan>:
//   tables in LDS                       trace_group (top list in LDS, every leaf a top entry)
//   tables in memory, <= kMaxTop leaves trace_group (top list in LDS, nodes / geoms read from memory)
//   tables in memory, more leaves       trace_group_packet: all rays of a group start at the camera
// The LDS block is k_intersect's (pt_lds.h IntersectLds).
template <bool TABLES_IN_LDS, bool PACKET>
__global__ __launch_bounds__(kBlock) void k_features(SceneTables sc, ptd::Camera cam, BatchInfo b, float4* __restrict__ feat) {
  static_assert(!(TABLES_IN_LDS && PACKET), "the packet scan reads the threaded tree with scalar loads from memory");
  extern __shared__ float4 lds_raw[];
  char* lds = reinterpret_cast<char*>(lds_raw);
  const IntersectLds L = intersect_lds<TABLES_IN_LDS>(sc);
  if (!PACKET) stage16(lds + L.top, sc.top, top_bytes(sc));
  const float4* top = reinterpret_cast<const float4*>(lds + L.top);
  const ptd::Node* nodes = sc.nodes;
  const ptd::Geom* geoms = sc.geoms;
  if (TABLES_IN_LDS) {
    stage16(lds + L.nodes, sc.nodes, node_bytes(sc));
    stage16(lds + L.geoms, sc.geoms, geom_bytes(sc));
    nodes = reinterpret_cast<const ptd::Node*>(lds + L.nodes);
    geoms = reinterpret_cast<const ptd::Geom*>(lds + L.geoms);
  }
  __syncthreads();
  const int wib = threadIdx.x >> 6;
  const WaveLds w = wave_lds_init(lds + L.waves + wib * L.wave_bytes);
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + wib);
  const int waves = gridDim.x * kWavesPerBlock;
  const int groups = (b.N + 63) >> 6;
  const float inv_w = 1.0f / (float)cam.res_x;
  const f3 o = mk(cam.pos[0], cam.pos[1], cam.pos[2]);
  const bool tri = sc.has_triangles != 0;
  float4* plane0 = feat;
  float4* plane1 = feat + (int64_t)b.N;
  float4* plane2 = feat + 2 * (int64_t)b.N;
  for (int g = wave; g < groups; g += waves) {
    const int pl_raw = g * 64 + lane;
    const bool valid = pl_raw < b.N;
    const int pl = valid ? pl_raw : b.N - 1;  // tile pixel
    const int p = global_pixel(b, pl);        // global pixel index
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0;
    if (valid) s0 = plane0[pl], s1 = plane1[pl], s2 = plane2[pl];
    // the current iteration's values: zeros on a miss
    f3 vn = mk(0.f, 0.f, 0.f), vp = vn, vc = vn;
    float vt = 0.f, vh = 0.f;
    int id = 0;
    for (int k = 0; k < b.K; ++k) {
      if (k == 0 || b.aa_jitter) {
        float jx = 0.f, jy = 0.f;
        if (b.aa_jitter) aa_jitter(b.iter_first + k, p, jx, jy);
        const f3 d = Ar<kD0>::camera_dir(cam, inv_w, p, b.aa_jitter != 0, jx, jy);
        if (PACKET) trace_group_packet<kD0>(w, nodes, sc.num_nodes, geoms, o, d, valid, lane, tri);
        else trace_group<kD0>(w, top, sc.num_top, nodes, geoms, o, d, valid, lane, sc.cull_margin, sc.top_xor, tri);
        const Hit h = resolve_hit(w.best[lane], w.rec + lane, valid, LeafGeom<>{nodes, geoms});
        vn = h.n, vp = h.p, vc = mk(0.f, 0.f, 0.f);
        vt = vh = 0.f;
        id = 0;
        if (h.hit) {
          const float* col = sc.mats[h.mat].color;
          vt = h.t;
          vh = 1.0f;
          vc = mk(col[0], col[1], col[2]);
          id = h.geom + 1;
        }
      }
      s0.x = s0.x + vn.x, s0.y = s0.y + vn.y, s0.z = s0.z + vn.z, s0.w = s0.w + vt;
      s1.x = s1.x + vc.x, s1.y = s1.y + vc.y, s1.z = s1.z + vc.z, s1.w = s1.w + vh;
      s2.x = s2.x + vp.x, s2.y = s2.y + vp.y, s2.z = s2.z + vp.z;
    }
    s2.w = __int_as_float(id);  // the LAST iteration's object: 1 + geom index, 0 = miss
    if (valid) plane0[pl] = s0, plane1[pl] = s1, plane2[pl] = s2;
  }
}
