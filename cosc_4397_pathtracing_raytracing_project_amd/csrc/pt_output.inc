// pt_output.inc — finalGather from the retirement records (k_collect), live-ray statistics, preview and 8-bit output kernels.
// Included by pt_kernels.hip inside ptk::<arith>::(anonymous).
// ───────────────────────────── gather / stats / preview ────────────────────
// finalGather (pathtrace.cu:439-444) from the retirement records: one workgroup per queue.  The queue owns the same
// pixels in every iteration (ptd::Queues), at most kCollectPixels of them per pass; for k = 0, 1, ... region (q, k) — one
// record per pixel of the queue, contiguous, exactly full (pt_device.h RetireBuf) — is read front to back with coalesced
// 16-byte loads and dropped into an LDS tile indexed by pixel, and every thread adds the tile to the accumulators of its
// pixels: image[p] = (((image[p] + c_0) + c_1) + ...), the order in which successive finalGather launches would have added
// them.  Nothing is scattered through memory: the regions are read once, the image is read and written once.  Queues
// with more pixels than a tile (frames beyond 4K at Q = 256 .. 1024) take several passes over their records.
constexpr int kCollectThreads = 1024;
constexpr int kCollectPPT = 8;                                // pixels (and records) per thread and pass
constexpr int kCollectPixels = kCollectPPT * kCollectThreads;  // 8192 pixels = 128 chunks: 96 KB of LDS
// (+ one int per residue: the sub-regions' depth-0 retiree counts of a BatchInfo::retire_once batch, collect_front_bits)
__host__ __device__ inline int collect_lds_bytes(int wq0) { return kCollectPixels * 12 + wq0 * 4; }
// records i0 + t, i0 + t + 1024, ... of a region, eight per thread
struct CollectChunk {
  ptd::Word4 v[kCollectPPT];
};
// (the u-th record of a thread exists only while i0 + u * 1024 < n — block-uniform: a queue of a small tile, e.g. 1024 pixels when
// eight GPUs share a 1080p frame, pays for one record per thread and iteration, not for eight)
// (FRESH: the record indices are formed anew at every call instead of living in sixteen registers across the iteration loop — the
// convergence variant needs those for the reference frame)
// (skip: bit u set — the thread's u-th record is neither loaded nor scattered, c.v[u] keeps whatever it held)
template <bool FRESH = false>
PT_DEV void collect_load(const ptd::Word4* rec, int n, int i0, uint32_t skip, CollectChunk& c) {
  int t = (int)threadIdx.x;
  if constexpr (FRESH) asm volatile("" : "+v"(t));
#pragma unroll
  for (int u = 0; u < kCollectPPT; ++u) {
    if (u > 0 && i0 + u * kCollectThreads >= n) break;
    const int i = i0 + u * kCollectThreads + t;
    if (!(skip >> u & 1u)) c.v[u] = rec[i < n ? i : (n > 0 ? n - 1 : 0)];
  }
}
// BatchInfo::retire_once (pt_sched.h): bit u set — the thread's u-th record of the chunk at i0 lies in a depth-0 retiree slot, the
// front of its sub-region.  In such a batch the slot holds the same colour for the same pixel in every iteration and is written in
// iteration 0 only: from iteration 1 on it is skipped and the tile keeps the pixel's value.  front[rho]: retirees of sub-region
// (q, 0, rho), in LDS; quo, rem: the queue's chunks over the residues (sub_slot).
PT_DEV uint32_t collect_front_bits(const int* front, int quo, int rem, int n, int i0) {
  uint32_t bits = 0;
#pragma unroll 1  // (two divisions per record: one after the other, their temporaries in the same registers)
  for (int u = 0; u < kCollectPPT; ++u) {
    if (u > 0 && i0 + u * kCollectThreads >= n) break;
    const int i = i0 + u * kCollectThreads + (int)threadIdx.x;
    if (i < n) {
      const SubSlot s = sub_slot(quo, rem, i);
      bits |= (retiree_slot(s, front[s.rho]) ? 1u : 0u) << u;
    }
  }
  return bits;
}
// (g0, g1: slots of the region that hold no record — the unused tail of the sub-region with the tile's partial last chunk)
PT_DEV void collect_scatter(const CollectChunk& c, int n, int i0, uint32_t skip, int g0, int g1, int Q, float inv_q, int first, float* tile) {
#pragma unroll
  for (int u = 0; u < kCollectPPT; ++u) {
    if (u > 0 && i0 + u * kCollectThreads >= n) break;
    const int i = i0 + u * kCollectThreads + (int)threadIdx.x;
    const int pl = __float_as_int(c.v[u].w);
    int jj, qq;
    divmod(pl >> 6, Q, inv_q, jj, qq);
    const int li = jj * 64 + (pl & 63) - first;
    if (i < n && !(skip >> u & 1u) && !(i >= g0 && i < g1) && li >= 0 && li < kCollectPixels) tile[3 * li] = c.v[u].x, tile[3 * li + 1] = c.v[u].y, tile[3 * li + 2] = c.v[u].z;
  }
}
// Convergence metric (PtOptions.convergence, ConvInfo in pt_kernels.h): after the adds of iteration k a thread holds the SUM image the
// reference has after iteration iter_first + k, so the squared error of computePSNR (pathtrace.cu:184-201) against the reference
// frame is taken right here — cur = sum / float(iteration) correctly rounded, d = cur - ref, d.x d.x + d.y d.y + d.z d.z without
// contraction in every build (namespace ex), added up in double.  The frame's values of a thread's pixels are loaded once per pass
// (or, when the frame is iteration capture_k of this very batch, taken from `cur` as it passes and stored); a wave adds its lanes'
// sums with cross-lane operations (wave_sum_f64) and one lane writes partial[k][queue][wave] — plain stores, a fixed order, no atomics, no barrier
// of its own.  k_conv_reduce adds the partials of an iteration.
constexpr int kCollectWaves = kCollectThreads / 64;
static_assert(kCollectWaves == kConvWaves, "the host sizes the partial sums with pt_kernels.h kConvWaves");
// Every one of three sums is +0 or lies in ieee::div_range (2^-47 <= v < 2^47): operands for which ieee::quot_core is the compiler's
// correctly rounded quotient (a sum of radiance is +0 before the first light reaches the pixel; 0 * r and the residuals stay +0).
// On the bit patterns, as unsigned numbers: the largest is below the pattern of 2^47 (which no negative number is) and the smallest
// of (pattern - 1) is at least the pattern of 2^-47 minus one (0 - 1 wraps to the top).  Denormal, huge, negative or non-finite
// sums send the wave through the compiler's divide.
PT_DEV bool conv_div_ok(float x, float y, float z) {
  const uint32_t a = __float_as_uint(x), b = __float_as_uint(y), c = __float_as_uint(z);
  return max(max(a, b), c) < 0x57000000u && min(min(a - 1u, b - 1u), c - 1u) >= 0x28000000u - 1u;
}
// The sum of a double over the wave's 64 lanes, wave-uniform, in a fixed order: four DPP steps leave the sum of each 16-lane row in
// all of its lanes (both partners of a step add the same two values), the four row sums are read into scalar registers and added
// front to back.  (~20 instructions; six dependent rounds of ds_bpermute pairs, as __shfl_xor would issue them, cost the gather of a
// small tile — one pixel per thread, 195 iterations per batch — more than everything else the metric does.)
template <int CTRL>
PT_DEV double dpp_f64(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xf, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, false);
  return __longlong_as_double((long long)((unsigned long long)hi << 32 | lo));
}
PT_DEV double readlane_f64(double v, int lane) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), lane);
  return __longlong_as_double((long long)((unsigned long long)hi << 32 | lo));
}
PT_DEV double wave_sum_f64(double v) {
  v += dpp_f64<0xb1>(v);   // quad_perm [1, 0, 3, 2]
  v += dpp_f64<0x4e>(v);   // quad_perm [2, 3, 0, 1]
  v += dpp_f64<0x141>(v);  // row_half_mirror
  v += dpp_f64<0x140>(v);  // row_mirror
  return ((readlane_f64(v, 0) + readlane_f64(v, 16)) + readlane_f64(v, 32)) + readlane_f64(v, 48);
}
// (ONCE: a BatchInfo::retire_once batch; a template parameter, so that every other batch runs the gather without the skip tests)
template <bool CONV, bool ONCE>
PT_DEV void collect_body(BatchInfo b, ptd::Queues qs, ptd::RetireBuf ret, float* __restrict__ image, ConvInfo cv) {
  extern __shared__ float4 lds_raw[];
  float* tile = reinterpret_cast<float*>(lds_raw);  // [kCollectPixels][3]
  const int q = blockIdx.x;
  const QueueShare sh = queue_share(b, qs, q);
  const float inv_q = 1.0f / (float)qs.Q;
  const ptd::Word4* rec = ret.rec + (int64_t)q * ret.kmax * ret.seg_cap;  // region (q, 0)
  // Records per region: flat form — my_pixels, appended from the front; otherwise one slot per pixel of the queue's my_nq chunks,
  // every one filled except the last (64 - N % 64) slots of the sub-region that holds the tile's partial last chunk.
  const int n = b.flat ? sh.my_pixels : sh.my_nq * 64;
  const auto [g0, g1] = b.flat ? Gap{0, 0} : region_gap(sh, ret.wq0);
  // BatchInfo::retire_once: the depth-0 retiree counts of the queue's sub-regions, row k = 0 of its sub[] (the rows of such a batch
  // are equal by construction), staged once per block behind the tile
  constexpr bool once = ONCE;
  int* front = reinterpret_cast<int*>(tile + 3 * kCollectPixels);  // [wq0]
  const int quo = once ? sh.my_nq / ret.wq0 : 0, rem = once ? sh.my_nq % ret.wq0 : 0;
  if (once) {
    for (int rho = threadIdx.x; rho < ret.wq0; rho += kCollectThreads) front[rho] = (int)(ret.sub[(int64_t)q * ret.kmax * ret.wq0 + rho] >> 32);
    __syncthreads();
  }
  for (int first = 0; first < sh.my_nq * 64; first += kCollectPixels) {  // one pass per kCollectPixels of the queue's pixels
    float acc[kCollectPPT][3];
    float rf[CONV ? kCollectPPT : 1][3];  // the reference frame's values of this thread's pixels
    uint32_t mine_bits = 0;               // bit m: pixel m of this thread exists (CONV); bit 8 + u: its u-th record of a region's first chunk is a
                                          // depth-0 retiree slot of a retire_once batch — formed once per pass, one register for both
    if (once) mine_bits = collect_front_bits(front, quo, rem, n, 0) << 8;
    // thread t owns the queue pixels first + t + kCollectThreads * m: chunk jj = index >> 6 is tile chunk q + jj * Q
#pragma unroll
    for (int m = 0; m < kCollectPPT; ++m) {
      const int li = first + threadIdx.x + kCollectThreads * m;
      const int pl = slot_pixel(q, li, qs.Q);
      const bool mine = li < sh.my_nq * 64 && pl < b.N;
      acc[m][0] = mine ? image[3 * (int64_t)pl] : 0.f, acc[m][1] = mine ? image[3 * (int64_t)pl + 1] : 0.f, acc[m][2] = mine ? image[3 * (int64_t)pl + 2] : 0.f;
      if constexpr (CONV) {
        const bool have = mine && cv.first_k == 0;  // the frame exists before this batch
        mine_bits |= (mine ? 1u : 0u) << m;
        rf[m][0] = have ? cv.ref[3 * (int64_t)pl] : 0.f, rf[m][1] = have ? cv.ref[3 * (int64_t)pl + 1] : 0.f, rf[m][2] = have ? cv.ref[3 * (int64_t)pl + 2] : 0.f;
      }
    }
    // software pipeline: the first 8192 records of iteration k + 1 are in flight while iteration k is summed (the tile is
    // reused every iteration, so the two barriers per iteration stay)
    CollectChunk c;
    // Iteration 0 of a pass loads and scatters the whole region, so every pixel of the window has its value in the tile and nothing
    // of an earlier pass or batch is used; the later iterations leave out the retiree slots (all of them: nothing is left out
    // unless retire_once).  acc += tile runs for every pixel in every iteration: the summation order is the same.
    collect_load<CONV>(rec, n, 0, 0u, c);
    for (int k = 0; k < b.K; ++k) {
      collect_scatter(c, n, 0, once && k > 0 ? mine_bits >> 8 : 0u, g0, g1, qs.Q, inv_q, first, tile);
      for (int i0 = kCollectPixels; i0 < n; i0 += kCollectPixels) {  // regions longer than one chunk (several passes only)
        const uint32_t skip = once && k > 0 ? collect_front_bits(front, quo, rem, n, i0) : 0u;  // (formed afresh: a rare form)
        collect_load<CONV>(rec + (int64_t)k * ret.seg_cap, n, i0, skip, c);
        collect_scatter(c, n, i0, skip, g0, g1, qs.Q, inv_q, first, tile);
      }
      if (k + 1 < b.K) collect_load<CONV>(rec + (int64_t)(k + 1) * ret.seg_cap, n, 0, once ? mine_bits >> 8 : 0u, c);
      __syncthreads();
#pragma unroll
      for (int m = 0; m < kCollectPPT; ++m) {
        if (m > 0 && first + kCollectThreads * m >= sh.my_nq * 64) break;  // block-uniform: pixels the queue does not have
        const int li = threadIdx.x + kCollectThreads * m;  // every pixel of the queue retires exactly once per iteration: no stale entries are read
        acc[m][0] += tile[3 * li], acc[m][1] += tile[3 * li + 1], acc[m][2] += tile[3 * li + 2];
      }
      if constexpr (CONV) {
        if (k == cv.capture_k || k >= cv.first_k) {  // block-uniform
          // 1 .. 2^24: inside ieee::div_range; divisor and refined reciprocal are the same in every lane: scalar registers
          const float n_it = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint((float)(b.iter_first + k))));
          uint32_t ok = 1u;
#pragma unroll
          for (int m = 0; m < kCollectPPT; ++m) {
            if (m > 0 && first + kCollectThreads * m >= sh.my_nq * 64) break;
            ok &= (~mine_bits >> m & 1u) | (uint32_t)conv_div_ok(acc[m][0], acc[m][1], acc[m][2]);
          }
          const bool short_div = ieee::every_lane(ok != 0u);
          const float r_it = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(ieee::rcp_core(n_it))));
          double sum = 0.0;
#pragma unroll
          for (int m = 0; m < kCollectPPT; ++m) {
            if (m > 0 && first + kCollectThreads * m >= sh.my_nq * 64) break;
            const bool mine = mine_bits >> m & 1u;
            f3 cur;
            if (short_div) cur = mk(ieee::quot_core(acc[m][0], n_it, r_it), ieee::quot_core(acc[m][1], n_it, r_it), ieee::quot_core(acc[m][2], n_it, r_it));
            else cur = mk(acc[m][0] / n_it, acc[m][1] / n_it, acc[m][2] / n_it);
            if (k == cv.capture_k) {
              rf[m][0] = cur.x, rf[m][1] = cur.y, rf[m][2] = cur.z;
              int t_cap = (int)threadIdx.x;
              asm volatile("" : "+v"(t_cap));  // the frame's addresses are formed here, once per render, not kept across the iteration loop
              const int li = first + t_cap + kCollectThreads * m;
              const int pl = slot_pixel(q, li, qs.Q);
              if (mine) cv.ref[3 * (int64_t)pl] = cur.x, cv.ref[3 * (int64_t)pl + 1] = cur.y, cv.ref[3 * (int64_t)pl + 2] = cur.z;
            } else {
              const f3 d = ex::sub(cur, mk(rf[m][0], rf[m][1], rf[m][2]));
              sum += mine ? (double)ex::dot(d, d) : 0.0;
            }
          }
          if (k >= cv.first_k) {
            sum = wave_sum_f64(sum);
            double* slot = cv.partial + ((int64_t)k * qs.Q + q) * kCollectWaves + (threadIdx.x >> 6);
            if ((threadIdx.x & 63) == 0) *slot = first == 0 ? sum : *slot + sum;  // (a later pass: this lane wrote the slot itself)
          }
        }
      }
      __syncthreads();
    }
    int t_out = (int)threadIdx.x;
    if constexpr (CONV) asm volatile("" : "+v"(t_out));  // the pixels' addresses are formed anew instead of living across the iteration loop
#pragma unroll
    for (int m = 0; m < kCollectPPT; ++m) {
      const int li = first + t_out + kCollectThreads * m;
      const int pl = slot_pixel(q, li, qs.Q);
      if (li < sh.my_nq * 64 && pl < b.N) image[3 * (int64_t)pl] = acc[m][0], image[3 * (int64_t)pl + 1] = acc[m][1], image[3 * (int64_t)pl + 2] = acc[m][2];
    }
  }
  // the records are consumed: zero counters for the next batch
  for (int i = threadIdx.x; i < ret.kmax; i += kCollectThreads) ret.cnt[(int64_t)q * ret.kmax + i] = 0ull;
}
__global__ __launch_bounds__(kCollectThreads) void k_collect(BatchInfo b, ptd::Queues qs, ptd::RetireBuf ret, float* __restrict__ image) {
  if (b.retire_once && !b.flat) collect_body<false, true>(b, qs, ret, image, ConvInfo{});
  else collect_body<false, false>(b, qs, ret, image, ConvInfo{});
}
// the same gather with the convergence metric: 4 waves per SIMD as well, i.e. at most 128 VGPRs
__global__ __launch_bounds__(kCollectThreads) void k_collect_conv(BatchInfo b, ptd::Queues qs, ptd::RetireBuf ret, float* __restrict__ image, ConvInfo cv) {
  if (b.retire_once && !b.flat) collect_body<true, true>(b, qs, ret, image, cv);
  else collect_body<true, false>(b, qs, ret, image, cv);
}
// sse[iteration - 1] = the partial sums of iteration iter_first + k, k = first_k + blockIdx.x, in a fixed order: thread t adds
// elements t, t + 256, ... of the Q * kCollectWaves values, a wave its lanes, thread 0 the four waves.
__global__ __launch_bounds__(kBlock) void k_conv_reduce(int iter_first, int first_k, int count, const double* __restrict__ partial, double* __restrict__ sse) {
  const int k = first_k + blockIdx.x;
  const double* p = partial + (int64_t)k * count;
  double acc = 0.0;
  for (int i = threadIdx.x; i < count; i += kBlock) acc += p[i];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  __shared__ double part[kWavesPerBlock];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = part[0];
    for (int w = 1; w < kWavesPerBlock; ++w) t += part[w];
    sse[iter_first + k - 1] = t;
  }
}

// k_paths' waves for the next batch (ptd::Queues::deal): queue q gets one wave plus its share of the other W - Q by the time
// its waves spent in this batch — first[q] = q + floor((W - Q) * work[0 .. q) / work[0 .. Q)), so every queue keeps a wave and
// first[Q] = W.  One block; the work counters are left zeroed.  Nothing measured, queues within the rounding of each other,
// or a Q this block has no room for: first[Q] = 0, which no launch width equals, i.e. W / Q waves each.
constexpr int kDealMaxQ = 2048;
PT_DEV void deal_waves(const ptd::Queues& qs) {
  __shared__ int work[kDealMaxQ];
  if (qs.deal == nullptr) return;
  const DealMap dm = deal_map(qs);
  if (threadIdx.x == 0) qs.deal[dm.strand_counter()] = 0;
  for (int q = threadIdx.x; q < qs.Q; q += blockDim.x) qs.deal[dm.piece_counter(q)] = 0;
  int32_t* first = qs.deal + dm.first(0);
  int32_t* wk = qs.deal + dm.time(0);
  const int Q = qs.Q, W = qs.paths_W;
  if (Q > kDealMaxQ || W < Q) {
    if (threadIdx.x == 0) qs.deal[dm.made_for()] = 0;
    for (int q = threadIdx.x; q < Q; q += blockDim.x) wk[q] = 0, qs.deal[dm.rays(q)] = 0;
    return;
  }
  // Whether to deal at all is decided by the RAYS the queues' paths cost (a property of the tile: the same in every batch), how by
  // the TIME their waves took: queues closer together in rays than the rounding of whole waves (heaviest / mean <= 1 + Q / W: a
  // whole 1080p frame, 1.03-1.04) keep W / Q waves each.
  __shared__ unsigned long long ray_total_s;
  __shared__ int ray_heaviest_s;
  if (threadIdx.x == 0) ray_total_s = 0ull, ray_heaviest_s = 0;
  __syncthreads();
  {
    int32_t* rays = qs.deal + dm.rays(0);
    unsigned long long sum = 0;
    int hv = 0;
    for (int q = threadIdx.x; q < Q; q += blockDim.x) sum += (unsigned long long)rays[q], hv = max(hv, rays[q]), rays[q] = 0;
    atomicAdd(&ray_total_s, sum);
    atomicMax(&ray_heaviest_s, hv);
  }
  for (int q = threadIdx.x; q < Q; q += blockDim.x) work[q] = wk[q], wk[q] = 0;
  __syncthreads();
  const bool close_together = queues_close_together(ray_heaviest_s, ray_total_s, W, Q);
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    unsigned long long total = 0;
    for (int e0 = 0; e0 < Q; e0 += 64) {
      unsigned long long v = e0 + lane < Q ? (unsigned long long)work[e0 + lane] : 0ull;
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      total += v;
    }
    if (close_together) total = 0;
    unsigned long long before = 0;  // work of the queues in front of this chunk
    for (int e0 = 0; e0 < Q && total > 0; e0 += 64) {
      const unsigned long long mine = e0 + lane < Q ? (unsigned long long)work[e0 + lane] : 0ull;
      unsigned long long incl = mine;
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
      }
      if (e0 + lane < Q) first[e0 + lane] = dealt_first(e0 + lane, W, Q, before + incl - mine, total);
      before += __shfl(incl, 63, 64);
    }
    if (lane == 0) qs.deal[dm.made_for()] = total > 0 ? W : 0;
  }
}

// one block per counter row (d = 0 .. depth_count): add the row's fill levels to the statistics and leave the
// row zeroed for the next batch (saves a memset launch per batch); block depth_count + 1 deals k_paths' waves
PT_DEV void count_stats_row(const ptd::Queues& qs, int32_t* __restrict__ cnt, int depth_count, unsigned long long* __restrict__ stats, int d) {
  if (d == depth_count + 1) {
    deal_waves(qs);
    return;
  }
  if (d > depth_count) return;
  unsigned long long acc = 0;
  for (int q = threadIdx.x; q < qs.Q; q += blockDim.x) {
    int32_t* c = &cnt[cnt_index(qs, d, q)];
    acc += (unsigned long long)*c;
    *c = 0;
  }
  if (d == depth_count) return;  // the row behind the last depth only needs the reset
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ unsigned long long part[kWavesPerBlock];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += part[w];
    stats[d] += t;
  }
}
__global__ void k_count_stats(ptd::Queues qs, int32_t* __restrict__ cnt, int depth_count,
                              unsigned long long* __restrict__ stats) {
  count_stats_row(qs, cnt, depth_count, stats, blockIdx.x);
}

// finalGather of a batch with fixed record slots (BatchInfo::fixed_slots, pt_sched.h): slot s of region (q, k) holds the same pixel for
// every k, so the gather is a plain stream — one thread per slot of the queue's region 0, `per_queue` blocks of kBlock per queue, no
// tile, no barrier.  Once per thread: the slot's sub-region and position there (sub_slot), the sub-region's depth-0 retiree count
// (row 0 of sub[]: the rows of such a batch are equal), the unused slots of the tile's partial last chunk (region_gap), and the pixel
// from the last word of the slot's record of iteration 0.  A survivor slot adds its K records to the pixel's accumulator strictly in
// iteration order — image[p] = (((image[p] + c_0) + c_1) + ...), k_collect's order — with kStreamGroup coalesced 16-byte loads in flight;
// a depth-0 retiree slot holds ONE record per batch (retire_once) and adds it K times, as the tile gather does from the value its tile
// keeps.  The blocks behind the gather's are k_count_stats' (count_stats_row): they touch the counter rows, the deal table and the
// statistics, the gather the records, sub[], ret.cnt and the image — nothing in common, so the batch saves a launch.
constexpr int kStreamGroup = 8;
// What one thread of the stream gather does for slot s of its queue — k_collect_stream's body, and a lane's share of a step of the gather
// k_paths runs for the batch before its own (pt_kernels.hip, PrevGather).  sh: the queue's share of the tile; K: the iterations of the batch
// that wrote the records; plane: the record plane that batch's k_paths wrote; front: plane 0, where k_primary leaves the depth-0
// retirees' records once per camera (the standalone gather of a batch in plane 0 passes the same plane twice).  GROUP: loads in flight.
template <int GROUP>
PT_DEV void stream_gather_slot(int N, int K, const QueueShare& sh, const ptd::RetireBuf& ret, const ptd::Word4* plane, const ptd::Word4* front,
                               float* __restrict__ image, int q, int s) {
  const Gap gap = region_gap(sh, ret.wq0);
  if (s >= sh.my_nq * 64 || (s >= gap.g0 && s < gap.g1)) return;
  const SubSlot ss = sub_slot(sh.my_nq / ret.wq0, sh.my_nq % ret.wq0, s);
  const int retirees = (int)(ret.sub[(int64_t)q * ret.kmax * ret.wq0 + ss.rho] >> 32);
  const bool once = retiree_slot(ss, retirees);
  const ptd::Word4* rec = (once ? front : plane) + (int64_t)q * ret.kmax * ret.seg_cap + s;  // the slot in region (q, 0); region (q, k): + k * seg_cap
  const ptd::Word4 r0 = rec[0];
  const int pl = __float_as_int(r0.w);
  if (pl < 0 || pl >= N) return;  // (no record names a pixel outside the tile; a slot nobody wrote must not send a store there)
  float* px = image + 3 * (int64_t)pl;
  float a0 = px[0], a1 = px[1], a2 = px[2];
  if (once) {
    for (int k = 0; k < K; ++k) a0 += r0.x, a1 += r0.y, a2 += r0.z;
  } else {
    a0 += r0.x, a1 += r0.y, a2 += r0.z;
    for (int k0 = 1; k0 < K; k0 += GROUP) {  // (K is uniform: the loads of a group are issued back to back, the last group's clamped)
      ptd::Word4 v[GROUP];
#pragma unroll
      for (int u = 0; u < GROUP; ++u) v[u] = rec[(int64_t)min(k0 + u, K - 1) * ret.seg_cap];
#pragma unroll
      for (int u = 0; u < GROUP; ++u) {
        const bool have = k0 + u < K;
        a0 = have ? a0 + v[u].x : a0, a1 = have ? a1 + v[u].y : a1, a2 = have ? a2 + v[u].z : a2;
      }
    }
  }
  px[0] = a0, px[1] = a1, px[2] = a2;
}
__global__ __launch_bounds__(kBlock) void k_collect_stream(BatchInfo b, ptd::Queues qs, ptd::RetireBuf ret, float* __restrict__ image, int per_queue,
                                                           int32_t* __restrict__ cnt, int depth_count, unsigned long long* __restrict__ stats) {
  const int gather_blocks = qs.Q * per_queue;
  if ((int)blockIdx.x >= gather_blocks) {
    count_stats_row(qs, cnt, depth_count, stats, (int)blockIdx.x - gather_blocks);
    return;
  }
  const int q = (int)blockIdx.x / per_queue, blk = (int)blockIdx.x - q * per_queue;
  const int s = blk * kBlock + (int)threadIdx.x;
  // the records are consumed: zero counters for the next batch
  if (blk == 0)
    for (int i = threadIdx.x; i < ret.kmax; i += kBlock) ret.cnt[(int64_t)q * ret.kmax + i] = 0ull;
  stream_gather_slot<kStreamGroup>(b.N, b.K, queue_share(b, qs, q), ret, ret.rec, ret.rec, image, q, s);
}
// The same gather for a batch whose k_paths wrote the second record plane (ret.rec; plane0: where the depth-0 retirees' records lie), without
// the counter rows' blocks: the last batch of a render call when it ends up in that plane, and a batch whose successor could not take it.
__global__ __launch_bounds__(kBlock) void k_collect_stream_planes(BatchInfo b, ptd::Queues qs, ptd::RetireBuf ret, const ptd::Word4* __restrict__ plane0,
                                                                  float* __restrict__ image, int per_queue) {
  const int q = (int)blockIdx.x / per_queue, blk = (int)blockIdx.x - q * per_queue;
  const int s = blk * kBlock + (int)threadIdx.x;
  if (blk == 0)
    for (int i = threadIdx.x; i < ret.kmax; i += kBlock) ret.cnt[(int64_t)q * ret.kmax + i] = 0ull;
  stream_gather_slot<kStreamGroup>(b.N, b.K, queue_share(b, qs, q), ret, ret.rec, plane0, image, q, s);
}

__global__ __launch_bounds__(kBlock) void k_preview(int n, int iterations, const float* __restrict__ image,
                                                    uchar4* __restrict__ rgba) {
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
    const float inv = (float)iterations;
    float v[3];
    for (int c = 0; c < 3; ++c) {
      const float pix = __builtin_powf(image[3 * (int64_t)p + c] / inv, 1.0f / 2.2f);
      int q = (int)(pix * 255.0f);
      v[c] = (float)(q < 0 ? 0 : (q > 255 ? 255 : q));
    }
    rgba[p] = make_uchar4((unsigned char)v[0], (unsigned char)v[1], (unsigned char)v[2], 0);
  }
}

// saveImage (main.cpp:86-107) + image::savePNG's conversion (image.cpp:22-39) on the device, for tiles made of whole
// image rows: tile pixel p = x + ty*W becomes three bytes at the x-mirrored position (W - 1 - x) + ty*W of its row,
// each (unsigned char)(clamp(sum / samples, 0, 1) * 255) — truncation, no gamma, NaN -> 0 like pt_image.cpp's to_u8.
// Write-out then moves 3 B per pixel over PCIe / xGMI instead of 12.
__global__ __launch_bounds__(kBlock) void k_save_u8(int n, int width, float samples, const float* __restrict__ image,
                                                    uint8_t* __restrict__ rgb8) {
  const float inv_w = 1.0f / (float)width;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
    int ty, x;
    divmod(p, width, inv_w, ty, x);
    uint8_t* dst = rgb8 + 3 * ((int64_t)ty * width + (width - 1 - x));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = image[3 * (int64_t)p + c] / samples;  // IEEE divide in every mode: bytes equal the host writer's
      float m = v > 0.0f ? v : 0.0f;
      m = m < 1.0f ? m : 1.0f;
      dst[c] = (uint8_t)(m * 255.f);
    }
  }
}
