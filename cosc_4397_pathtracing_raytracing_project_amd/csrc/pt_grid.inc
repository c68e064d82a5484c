// pt_grid.inc — uniform-grid walk of the fused kernels on large scenes (cell ring, leaf-box filter, 3D-DDA, grid_search).
// Included by pt_kernels.hip inside ptk::<arith>::(anonymous), after the candidate ring (Carry).
// ── uniform grid walk (SceneTables::grid_*; large scenes, when faster than the BVH scan) ───────────────────────────────
// Second ring of a wave: cell records a ray came across, waiting for their leaf-box test.  Entry: record index << 10 |
// direction the ray entered the cell from (0..5 = through its -x, +x, -y, +y, -z, +z face, 7 = first cell) << 7 |
// group parity << 6 | owner lane.
struct CellRing {
  uint32_t* ent;  // [kCellRing] (pt_lds.h)
  int head, count;
  float* rinv;    // [rinv_planes][64] reciprocal direction of each lane's ray in the mode's arithmetic (+ -o * that: fast)
};
// What the leaf-box tests need of a ray is computed once per ray and kept in LDS (CellRing::rinv) instead of once per record
// (a group tests ~950 records, 15 per ray): the reciprocal direction — three IEEE divides in the exact and fma arithmetic —
// and, where the slab test has the FMA form t = plane * i + n (fast), n = -o * i as well, so that a record's test reads six
// values and computes no reciprocal.  (Round 2 measured the stored reciprocals 34 % slower for the fast build of the kernel
// as it was then; round 3, with the retirement and filing changes in: 3.4 % faster, `n` included 6 %.)
struct GridRings {
  Carry<false, 1> cy;  // with gix
  CellRing cr;
};
template <bool EX>
PT_DEV GridRings grid_rings_init(char* base) {  // on a GridMap<kFast, EX>::bytes block
  using M = GridMap<kFast, EX>;
  GridRings g{carry_init<false, 1>(base), CellRing{reinterpret_cast<uint32_t*>(base + M::cells), 0, 0, reinterpret_cast<float*>(base + M::rinv)}};
  g.cy.gix = reinterpret_cast<uint32_t*>(base + M::gix);
  return g;
}
// Exclusive prefix sum over the wave of a small count per lane, and the total: a Hillis-Steele scan on the DPP network —
// four row_shr steps scan each row of 16 lanes, row_bcast:15 / :31 carry the row totals over — six v_add_u32_dpp instead of
// the six ballots + twelve mbcnt + six shift-adds of a bit-sliced count (round 2; the walk loop runs this once per cell step).
// All 64 lanes must be active (the callers' control flow is wave-uniform).
PT_DEV int wave_prefix6(int v, int& total) {
  int x = v;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);   // row_shr:1, zero shifted in
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);   // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);   // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);   // row_shr:8: inclusive scan of each row
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
  total = __builtin_amdgcn_readlane(x, 63);
  return x - v;
}
// Leaf-box tests (the mode's slab arithmetic: these decide, exactly like the reference's walk, which primitives a ray is
// tested against) for the first n (<= 64) pending records; passing leaves go to the primitive ring.  A leaf that is also
// listed in the cell the ray came from was handled there: a box occupies a block of cells and the ray's cells inside a
// block are consecutive.  Wave-uniform control flow.
template <int NPAR, bool EX = false>
PT_DEV void grid_filter(Carry<false, NPAR>& c, CellRing& cr, int n, const SceneTables& sc, int lane,
                        const ptd::Node* __restrict__ nodes, const ptd::Geom* __restrict__ geoms) {
  const bool valid = lane < n;
  PT_STAT(4, 1);
  PT_STAT(5, n);
  const uint32_t entry = cr.ent[(cr.head + lane) & (kCellRing - 1)];
  const int src = (int)(entry & 63u);
  const int par = (int)((entry >> 6) & 1u);
  const int from = (int)((entry >> 7) & 7u);
  const uint32_t item = valid ? entry >> 10 : 0u;
  const float4* items = reinterpret_cast<const float4*>(EX ? sc.grid_items : sc.grid_items_b);  // EX: primary rays on the reference's boxes
  const float4 NA = items[2 * item];      // bmin.xyz, bmax.x
  const float4 NB = items[2 * item + 1];  // bmax.yz, leaf, neighbour bits
  RayInv ri;  // as ray_inv() builds it, from the values stored once per ray
  f3 ro = mk(0.f, 0.f, 0.f);
  ri.ix = cr.rinv[0 * 64 + src], ri.iy = cr.rinv[1 * 64 + src], ri.iz = cr.rinv[2 * 64 + src];
  ri.sx = ri.ix < 0.0f, ri.sy = ri.iy < 0.0f, ri.sz = ri.iz < 0.0f;
  if (rinv_planes<kFast, EX>() == 6) {  // FMA form: the origin itself is not needed
    ri.nx = cr.rinv[3 * 64 + src], ri.ny = cr.rinv[4 * 64 + src], ri.nz = cr.rinv[5 * 64 + src];
  } else {
    const float* ray = c.ray + par * 6 * 64 + src;
    ro = mk(ray[0 * 64], ray[1 * 64], ray[2 * 64]);
    ri.nx = -ro.x * ri.ix, ri.ny = -ro.y * ri.iy, ri.nz = -ro.z * ri.iz;
  }
  const float bt = __uint_as_float(reinterpret_cast<const uint32_t*>(c.best)[2 * (par * 64 + src) + 1]) + sc.cull_margin;
  float tn;
  const uint32_t bits = __float_as_uint(NB.w);  // neighbour bits | primitive type << 6 | geom index << 8
  const bool seen = ((bits & 63u) >> from) & 1u;  // from == 7: first cell of a walk, nothing seen
  // no short-circuit: with `&&` the compiler fetches the record's last 8 bytes first, branches on `seen`, and only then fetches
  // the box — two dependent memory round trips per chunk and 2.6 load instructions per record instead of 2
  const bool box = Ar<EX>::slab_t(ro, ri, NA.x, NA.y, NA.z, NA.w, NB.x, NB.y, tn);
  const bool pass = (int)valid & (int)!seen & (int)box & (int)!(tn > bt);
  cr.head = (cr.head + n) & (kCellRing - 1);
  cr.count -= n;
#ifdef PT_WALK_STATS
  const int st_seen = __popcll(ballot(valid && seen)), st_pass = __popcll(ballot(pass));
  const int st_box = __popcll(ballot(valid && !seen && Ar<EX>::slab_t(ro, ri, NA.x, NA.y, NA.z, NA.w, NB.x, NB.y, tn)));
  PT_STAT(10, st_seen);
  PT_STAT(11, st_pass);
  PT_STAT(12, st_box);
#endif
  carry_append<false, NPAR, EX, true>(c, pass, __float_as_uint(NB.z), par, src, lane, nodes, geoms,
                                      (bits >> 8) | (((bits >> 6) & 3u) << 30));
}
// State of a lane's cell walk (3D-DDA): the distance along the ray of the next cell boundary per axis, the distance
// between boundaries, the current cell.  A walk ends by distance alone (te > t_end, the grid's far side): the boundary
// distances accumulate rounding, so the decision at the exit face can come a step late — up to three steps at a corner of
// the grid — and the cell index then leaves the grid by at most one cell per axis, i.e. by < rx * ry + rx + 2 entries of
// the cell table: the host pads the table with that many empty cells on both sides (pt_tables.cpp), and a wrapped index
// inside the table only adds records to test (round 2 counted the cells left per axis instead: 3 registers and 6
// instructions per step).
struct CellWalk {
  float tx, ty, tz, ddx, ddy, ddz;
  int px, py, pz;  // per axis: cell-index step << 3 | face the next cell is entered through (0..5 = its -x, +x, -y, +y, -z, +z face)
  int idx;
  float te, t_end;  // entry distance of the current cell; the walk covers [te, t_end]
  uint32_t from;    // face the current cell was entered through (grid_filter), 7: first cell of a walk
  int own;          // lane that owns the ray
  bool on;
};
// Start a walk of ray (o, d) over the part [t_from, t_to] of its span inside the grid.  Fast float arithmetic in every
// mode: the walk only has to reach every cell the ray touches, which the padding of the cell lists guarantees.
PT_DEV void walk_start(const SceneTables& sc, f3 o, f3 d, float t_from, float t_to, bool want, int own, CellWalk& w) {
  const float dx = __builtin_copysignf(__builtin_fmaxf(__builtin_fabsf(d.x), 1e-20f), d.x);
  const float dy = __builtin_copysignf(__builtin_fmaxf(__builtin_fabsf(d.y), 1e-20f), d.y);
  const float dz = __builtin_copysignf(__builtin_fmaxf(__builtin_fabsf(d.z), 1e-20f), d.z);
  const float ix = __builtin_amdgcn_rcpf(dx), iy = __builtin_amdgcn_rcpf(dy), iz = __builtin_amdgcn_rcpf(dz);
  const int rx = sc.grid_res[0], ry = sc.grid_res[1], rz = sc.grid_res[2];
  const float gx = sc.grid_min[0], gy = sc.grid_min[1], gz = sc.grid_min[2];
  const float csx = sc.grid_cs[0], csy = sc.grid_cs[1], csz = sc.grid_cs[2];
  const float ax0 = (gx - o.x) * ix, ax1 = (gx + csx * (float)rx - o.x) * ix;
  const float ay0 = (gy - o.y) * iy, ay1 = (gy + csy * (float)ry - o.y) * iy;
  const float az0 = (gz - o.z) * iz, az1 = (gz + csz * (float)rz - o.z) * iz;
  const float t_in = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(ax0, ax1), __builtin_fminf(ay0, ay1)),
                                     __builtin_fmaxf(__builtin_fminf(az0, az1), t_from));
  const float t_out = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(ax0, ax1), __builtin_fmaxf(ay0, ay1)),
                                      __builtin_fminf(__builtin_fmaxf(az0, az1), t_to));
  w.on = want && t_out >= t_in;
  const float px = o.x + d.x * t_in, py = o.y + d.y * t_in, pz = o.z + d.z * t_in;
  const int cx = min(max((int)__builtin_floorf((px - gx) * sc.grid_inv_cs[0]), 0), rx - 1);
  const int cy = min(max((int)__builtin_floorf((py - gy) * sc.grid_inv_cs[1]), 0), ry - 1);
  const int cz = min(max((int)__builtin_floorf((pz - gz) * sc.grid_inv_cs[2]), 0), rz - 1);
  const bool fx = dx >= 0.0f, fy = dy >= 0.0f, fz = dz >= 0.0f;  // moving towards +x / +y / +z
  w.tx = (gx + csx * (float)(cx + (fx ? 1 : 0)) - o.x) * ix;
  w.ty = (gy + csy * (float)(cy + (fy ? 1 : 0)) - o.y) * iy;
  w.tz = (gz + csz * (float)(cz + (fz ? 1 : 0)) - o.z) * iz;
  w.ddx = csx * __builtin_fabsf(ix), w.ddy = csy * __builtin_fabsf(iy), w.ddz = csz * __builtin_fabsf(iz);
  const int rxy = rx * ry;
  w.px = fx ? 8 + 0 : -8 + 1;  // moving +x: the next cell is entered through its -x face  (step = word >> 3, face = word & 7)
  w.py = fy ? 8 * rx + 2 : -8 * rx + 3;
  w.pz = fz ? 8 * rxy + 4 : -8 * rxy + 5;
  w.idx = cx + rx * (cy + ry * cz);
  w.te = t_in;
  w.t_end = t_out;
  w.from = 7u;
  w.own = own;
}
// Candidate search of one group through the grid: every lane walks its own ray cell by cell, files the records of each
// cell in the cell ring, and stops at the far side of the grid or once the next cell starts beyond the ray's best hit so
// far (the closer-hit cull of the subtree scans, same margin + the padding).  Rays hit after 6 cells on average but the
// longest of 64 walks takes 26, so once few lanes are still walking their remaining spans are cut into equal parts and
// dealt to all 64 lanes (candidates are filed under the lane that owns the ray, as with the work stealing of the
// subtree scans; the parts overlap by a cell, which costs a repeated test and changes nothing).
constexpr int kGridSplit = 16;  // lanes still walking when the remaining spans are dealt out
template <int NPAR, bool EX = false>
PT_DEV void grid_search(Carry<false, NPAR>& c, CellRing& cr, const SceneTables& sc, const ptd::Node* __restrict__ nodes,
                        const ptd::Geom* __restrict__ geoms, f3 o, f3 d, bool valid, int lane, int par) {
  float* rays = c.ray + par * 6 * 64;
  rays[0 * 64 + lane] = o.x, rays[1 * 64 + lane] = o.y, rays[2 * 64 + lane] = o.z;
  rays[3 * 64 + lane] = d.x, rays[4 * 64 + lane] = d.y, rays[5 * 64 + lane] = d.z;
  {
    const RayInv ri = Ar<EX>::ray_inv(d, o);
    cr.rinv[0 * 64 + lane] = ri.ix, cr.rinv[1 * 64 + lane] = ri.iy, cr.rinv[2 * 64 + lane] = ri.iz;
    if (rinv_planes<kFast, EX>() == 6) cr.rinv[3 * 64 + lane] = ri.nx, cr.rinv[4 * 64 + lane] = ri.ny, cr.rinv[5 * 64 + lane] = ri.nz;
  }
  CellWalk w;
  PT_STAT(0, 1);
  walk_start(sc, o, d, 0.0f, FLT_MAX, valid, lane, w);
  const float slack = sc.cull_margin + 2.0f * sc.grid_pad;
  int splits = 0;
  while (true) {
    const float bt = __uint_as_float(reinterpret_cast<const uint32_t*>(c.best)[2 * (par * 64 + w.own) + 1]) + slack;
    w.on = w.on && !(w.te > bt) && !(w.te > w.t_end);
    const unsigned long long M = ballot(w.on);
    if (!M) break;
    PT_STAT(1, 1);
    PT_STAT(2, __popcll(M));
    if (splits < 2 && __popcll(M) <= kGridSplit) {
      ++splits;
      const int n_on = __popcll(M);
      const int rank = rank_in(M);
      if (w.on) c.slot[rank] = lane;
      const int k = 64 / n_on;
      const int r = lane / k, seg = lane - r * k;
      const bool take = r < n_on;
      const int donor = c.slot[take ? r : 0];
      const float d_te = bperm(donor, w.te), d_end = bperm(donor, w.t_end);
      const int d_own = __builtin_amdgcn_ds_bpermute(donor << 2, w.own);
      const f3 so = mk(rays[0 * 64 + d_own], rays[1 * 64 + d_own], rays[2 * 64 + d_own]);
      const f3 sd = mk(rays[3 * 64 + d_own], rays[4 * 64 + d_own], rays[5 * 64 + d_own]);
      const float part = (d_end - d_te) / (float)k;
      const float ta = d_te + part * (float)seg;
      const float tb = seg == k - 1 ? d_end : ta + part;
      walk_start(sc, so, sd, ta, tb, take, d_own, w);
    }
    const uint2 se = w.on ? *reinterpret_cast<const uint2*>(sc.grid_start + w.idx) : make_uint2(0u, 0u);  // 4-byte aligned pair
    const uint32_t tag = (w.from << 7) | ((uint32_t)par << 6) | (uint32_t)w.own;
    // File the cells' records, a cell's records next to each other: the lanes of a box-test chunk then read neighbouring
    // 32-byte records (one L1 access per 128-byte line instead of one per lane — the L1's access rate is what bounds
    // this kernel).  Ring positions from a prefix sum over the lanes' list lengths; a step files at most 192 records at
    // once, a lane up to 63 (longer lists and later lanes take another turn).
    uint32_t it = se.x;
    while (true) {
      const int want = (int)min(se.y - it, 63u);
      int total;
      const int pre = wave_prefix6(want, total);
      if (total == 0) break;
      const bool now = pre + want <= kCellRing - 64;
      const int take = now ? want : 0;
#ifdef PT_WALK_STATS
      const int st_trips = wave_max_stat(take), st_lanes = __popcll(ballot(take > 0));
      PT_STAT(3, 1);
      PT_STAT(8, st_trips);
      PT_STAT(9, st_lanes);
#endif
      const int base = cr.head + cr.count + pre;
      for (int j = 0; j < take; ++j) cr.ent[(base + j) & (kCellRing - 1)] = ((it + (uint32_t)j) << 10) | tag;
      it += (uint32_t)take;
      // the lanes that filed are a prefix of the lanes (pre grows with the lane index): the last one knows the sum
      const unsigned long long nm = ballot(now);
      if (nm) cr.count += __builtin_amdgcn_readlane(pre + want, 63 - __builtin_clzll(nm));
      while (cr.count >= 64) grid_filter<NPAR, EX>(c, cr, 64, sc, lane, nodes, geoms);
      if (!ballot(it != se.y)) break;  // the usual case: every list went in at once — no second pass to find that out
    }
    // next cell: through the nearest boundary
    w.te = __builtin_fminf(__builtin_fminf(w.tx, w.ty), w.tz);
    const bool ax = w.tx == w.te;
    const bool ay = !ax && w.ty == w.te;
    const int step = ax ? w.px : ay ? w.py : w.pz;
    w.idx += step >> 3;
    w.from = (uint32_t)step & 7u;
    if (ax) w.tx += w.ddx;
    else if (ay) w.ty += w.ddy;
    else w.tz += w.ddz;
  }
  while (cr.count > 0) grid_filter<NPAR, EX>(c, cr, min(64, cr.count), sc, lane, nodes, geoms);
}
