// pt_sched.h — how work is dealt out: which wave traces which sample, and where a record or a counter lives.
//
// The kernels (pt_kernels.hip, pt_shade.inc, pt_output.inc) and the host (pt_api.cpp) take these numbers from here, so the
// two cannot disagree.  Plain C++ (the system compiler accepts it; tests/test_sched.py sweeps every function by enumeration):
// integer arithmetic on (N, Q, W, K, wq0, pieces) only, no pointers into device memory and no runtime calls — the structs
// that hold device pointers (Retire, the k_paths cursor) stay in pt_kernels.hip and take their offsets from here.
#pragma once
#include "pt_kernels.h"

#define PT_SCHED __host__ __device__ inline __attribute__((always_inline))

namespace ptk {

PT_SCHED int sched_min(int a, int b) { return a < b ? a : b; }
PT_SCHED int sched_max(int a, int b) { return a > b ? a : b; }

// ── ptd::Queues::deal: five regions of int32 words, back to back ──────────────────────────────────────────────────────────
//   first(0 .. Q)      first k_paths wave of queue q; word Q (= made_for()) holds the launch width W the table was made for
//                      (0: nothing measured, or queues close together) — any other launch width gets W / Q waves per queue
//   time(q)            time the waves of queue q spent in this batch's k_paths launch, 0.64-us units
//   strand_counter()   where k_primary's waves take the later pieces of the strands from
//   piece_counter(q)   where the waves of queue q take pieces of its depth-1 rays from in k_paths
//   rays(q)            rays the waves of queue q traced in k_paths
// k_count_stats (deal_waves) turns time / rays into the next batch's first[] and leaves everything else zeroed.
struct DealMap {
  int Q;
  PT_SCHED int first(int q) const { return q; }
  PT_SCHED int made_for() const { return Q; }
  PT_SCHED int time(int q) const { return Q + 1 + q; }
  PT_SCHED int strand_counter() const { return 2 * Q + 1; }
  PT_SCHED int piece_counter(int q) const { return 2 * Q + 2 + q; }
  PT_SCHED int rays(int q) const { return 3 * Q + 2 + q; }
  PT_SCHED int words() const { return 4 * Q + 2; }
};
PT_SCHED DealMap deal_map(const ptd::Queues& qs) { return DealMap{qs.Q}; }

// first[q] of the next batch: queue q gets one wave plus its share of the other W - Q by the work of the queues in front of
// it, so first[] is strictly increasing (every queue keeps a wave), first[0] = 0 and first[Q] = W.  (W >= Q, work_total > 0)
PT_SCHED int dealt_first(int q, int W, int Q, unsigned long long work_before, unsigned long long work_total) {
  return q + (int)((unsigned long long)(W - Q) * work_before / work_total);
}
// Queues closer together in rays than the rounding of whole waves (heaviest / mean <= 1 + Q / W) keep W / Q waves each.
PT_SCHED bool queues_close_together(int heaviest_rays, unsigned long long total_rays, int W, int Q) {
  return (unsigned long long)heaviest_rays * W * Q <= total_rays * ((unsigned long long)W + Q);
}

// ── queue geometry (pt_device.h Queues, RetireBuf) ────────────────────────────────────────────────────────────────────────
// Wave `wave` of a grid of W waves (a multiple of Q) serves queue q as the r-th of its wq waves.
struct WaveSlot {
  int q, r, wq;
};
PT_SCHED WaveSlot wave_slot(int wave, int Q, int W) { return WaveSlot{wave % Q, wave / Q, W / Q}; }

// Queue q's share of an iteration: chunks q, q + Q, ... of the tile's ceil(N / 64); only the tile's last chunk can be
// partial, and it is the last chunk of the queue that owns it.
struct QueueShare {
  int my_nq;      // chunks of this queue per iteration
  int my_pixels;  // pixels of this queue per iteration
  float inv_my_nq;
};
PT_SCHED QueueShare queue_share(const BatchInfo& b, const ptd::Queues& qs, int q) {
  const int chunks = (b.N + 63) >> 6;
  QueueShare sh;
  sh.my_nq = q < chunks ? (chunks - q + qs.Q - 1) / qs.Q : 0;
  const int last_q = (chunks - 1) % qs.Q;
  sh.my_pixels = sh.my_nq * 64 - ((q == last_q && (b.N & 63)) ? 64 - (b.N & 63) : 0);
  sh.inv_my_nq = sh.my_nq > 0 ? 1.0f / (float)sh.my_nq : 0.0f;
  return sh;
}
// First tile pixel of the queue's chunk jj (tile chunk q + jj * Q); lane l of a wave has pixel + l.
PT_SCHED int chunk_pixel(int q, int jj, int Q) { return (q + jj * Q) * 64; }
// Tile pixel of the queue's pixel slot li = jj * 64 + lane.
PT_SCHED int slot_pixel(int q, int li, int Q) { return chunk_pixel(q, li >> 6, Q) + (li & 63); }

// Sub-list / sub-region (q, k, rho) of a queue with my_nq chunks per iteration dealt to wq0 residues: c(rho) chunks, the first
// of them off(rho) chunks into list / region (q, k)  (residue rho owns the chunks jj = rho, rho + wq0, ...).
// (quo = my_nq / wq0, rem = my_nq % wq0, computed once per kernel)
PT_SCHED int sub_chunks(int quo, int rem, int rho) { return quo + (rho < rem ? 1 : 0); }
PT_SCHED int sub_offset(int quo, int rem, int rho) { return rho * quo + sched_min(rho, rem); }
// The record slots [g0, g1) of a region that stay unused: none when the queue's chunks are whole, otherwise the last
// 64 - N % 64 slots of the sub-region that holds the tile's partial last chunk (the queue's last chunk, my_nq - 1).
struct Gap {
  int g0, g1;
};
PT_SCHED Gap region_gap(const QueueShare& sh, int wq0) {
  Gap g{0, 0};
  const int missing = sh.my_nq * 64 - sh.my_pixels;
  if (missing > 0) {
    const int quo = sh.my_nq / wq0, rem = sh.my_nq % wq0, rho = (sh.my_nq - 1) % wq0;
    g.g1 = (sub_offset(quo, rem, rho) + sub_chunks(quo, rem, rho)) * 64;
    g.g0 = g.g1 - missing;
  }
  return g;
}

// The counter rows cnt[depth][Q], cnt_stride ints apart: the index of queue q's counter in row d, and the rows' words.
PT_SCHED size_t cnt_index(const ptd::Queues& qs, int d, int q) { return (size_t)qs.Q * qs.cnt_stride * d + (size_t)q * qs.cnt_stride; }

// What the host sizes the queues with: chunks per queue and iteration, record slots per region (queue, iteration), paths
// per queue and batch.
struct QueuePlan {
  int nq, seg_cap, cap;
};
PT_SCHED int chunks_per_queue(int64_t N, int Q) { return (int)(((N + 63) / 64 + Q - 1) / Q); }
PT_SCHED QueuePlan queue_plan(int64_t N, int Q, int K) {
  QueuePlan p;
  p.nq = chunks_per_queue(N, Q);
  p.seg_cap = p.nq * 64;
  p.cap = K * p.seg_cap;
  return p;
}
// Entries of RetireBuf::sub per region: the waves per queue of the widest k_primary grid.
PT_SCHED size_t sub_stride(int widest_grid_waves, int Q) { return (size_t)widest_grid_waves / Q; }

// ── k_primary: strands ────────────────────────────────────────────────────────────────────────────────────────────────────
// A strand = what one wave of one queue traces at depth 0: in iteration k the queue's chunks jj = rho, rho + wq, ... of
// residue rho = (r + k) mod wq.  The strands are cut into `pieces` runs of kp iterations; strand index s < W is piece 0 of
// wave s, the indices from W on (piece by piece, W each) go to whoever is free.  Every (queue, iteration, residue) has ONE owner.
struct StrandPlan {
  int kp, pieces;
};
PT_SCHED StrandPlan strand_plan(int K, int primary_pieces, bool deal_present, bool flat) {
  StrandPlan p;
  p.kp = primary_pieces > 1 && deal_present && !flat ? (K + primary_pieces - 1) / primary_pieces : K;
  p.pieces = (K + p.kp - 1) / p.kp;
  return p;
}
struct Strand {
  int piece, q, r, wq, k0, k1;  // iterations [k0, k1) of wave r of queue q's wq
};
PT_SCHED Strand strand_of(int strand, const StrandPlan& p, int K, int Q, int W) {
  Strand s;
  s.piece = strand / W;
  const WaveSlot w = wave_slot(strand - s.piece * W, Q, W);
  s.q = w.q, s.r = w.r, s.wq = w.wq;
  s.k0 = s.piece * p.kp, s.k1 = sched_min(K, s.k0 + p.kp);
  return s;
}
PT_SCHED int strand_rho(int r, int k, int wq) { return (r + k) % wq; }
PT_SCHED int strand_rho_before(int r, int k, int wq) { return (r + k + wq - 1) % wq; }  // rho of iteration k - 1 (k >= 0)
// The host's choice of primary_pieces: a piece pays for its own pipeline drain, so it should hold a few dozen 64-sample
// groups; a wave's strand has K * nq / (waves per queue) of them.
PT_SCHED int auto_primary_pieces(int K, int nq, int wq0) {
  const int64_t want = (int64_t)K * nq / sched_max(1, wq0) / 48;
  return want < 1 ? 1 : want > 4 ? 4 : (int)want;
}

// ── k_primary, shared form: one trace per chunk and run of iterations ──────────────────────────────────────────────────────
// Without anti-aliasing jitter a pixel's camera ray, and so its first hit, is the same in every iteration.  In the shared
// form a strand keeps ONE residue, rho = r in every iteration of its piece, so the wave meets the same chunks jj = r, r + wq,
// ... in all of them: it traces a chunk once and shades it for a run of iterations.  (queue, iteration k, residue rho) is
// then owned by (wave rho, piece containing k): still one owner, and for a fixed k the owner still appends its chunks in
// ascending jj, so every sub-list and sub-region holds what the per-iteration form puts there, in the same order.
// A run is at most kShareMax iterations (the per-iteration counters of a run live in the 64 lanes of two registers); a
// longer piece is walked as sub-runs, each tracing the chunks again.
constexpr int kShareMax = 64;
// Which form a batch runs: the shared one needs the camera rays to be the same in every iteration (no jitter) and the
// per-(queue, iteration) sub-lists (not flat); BatchInfo::primary_share <= 1 asks for a trace per iteration, and so does
// PtOptions.debug_flags kTraceEveryIteration (the host passes a primary_share of 1 then).  The first rung of batch_form, below.
constexpr int kTraceEveryIteration = 128;
PT_SCHED bool primary_shares(int primary_share, bool aa_jitter, bool flat) { return primary_share > 1 && !aa_jitter && !flat; }
PT_SCHED bool primary_shares(const BatchInfo& b) { return primary_shares(b.primary_share, b.aa_jitter != 0, b.flat != 0); }
PT_SCHED int shared_rho(int r, int /*k*/, int /*wq*/) { return r; }  // the strand's residue in iteration k: the same in all of them (beside strand_rho)
// Longest run per trace from BatchInfo::primary_share (<= 1: the per-iteration form, not this one).
PT_SCHED int shared_run_cap(int primary_share) { return primary_share < 1 ? 1 : sched_min(primary_share, kShareMax); }
// Sub-runs of the piece [k0, k1): i = 0 .. shared_runs() - 1 cover [k0 + i * cap, min(k1, k0 + (i + 1) * cap)).
struct Run {
  int k0, k1;
};
PT_SCHED int shared_runs(int k0, int k1, int cap) { return (k1 - k0 + cap - 1) / cap; }
PT_SCHED Run shared_run(int k0, int k1, int cap, int i) { return Run{k0 + i * cap, sched_min(k1, k0 + (i + 1) * cap)}; }
// The host's choice of primary_pieces for the shared form.  A wave with a fixed residue has quo or quo + 1 chunks in EVERY
// iteration (the per-iteration form's rotation evened that out over the batch), so the pieces behind the counter are what
// levels the waves, and each piece pays one trace per chunk.  Swept on the whole 1080p frame (K = 25) and on an eighth of it
// (K = 195), profiles/first_hit_sharing.log section 2b: 2 pieces win on the frame (1 / 2 / 4 / 8: 31.3 / 31.9 / 31.4 / 28.5 k
// Msamples/s), 4 on the eighth (29.5 / 29.9 / 30.2 / 26.8 k), where a piece of K / 4 = 49 iterations is still ONE run — a
// piece longer than kShareMax traces its chunks again anyway, so it may as well be a piece of its own: max(2, ceil(K / 64)).
PT_SCHED int auto_shared_pieces(int K, int /*nq*/, int /*wq0*/) {
  const int want = sched_max(2, (K + kShareMax - 1) / kShareMax);
  return sched_max(1, sched_min(want, K));
}

// ── depth-0 retirees: stored and gathered once per batch ──────────────────────────────────────────────────────────────────
// A sample that retires at depth 0 of a path with trace_depth >= 2 is a miss or an emitter hit: shade_decide (pt_shade.inc)
// returns for both before any draw of the iteration's RNG is used, roulette starts at depth 4, and every other hit survives
// while 1 < trace_depth.  With the same camera ray in every iteration (the shared form) WHETHER a pixel retires at depth 0, and
// the colour it retires with, are therefore functions of the pixel alone: the K records of a pixel are equal.  Such a batch
// (BatchInfo::retire_once) writes them in iteration 0 only and k_collect, whose LDS tile is indexed by pixel and survives from
// iteration to iteration, gathers them there only.  The layout is untouched: slots, counts and RetireBuf::sub stay what
// they are (so k_paths sees the same buffers); the retiree slots at the front of the sub-regions of iterations >= 1 are
// simply neither written nor read.  With trace_depth == 1 EVERY sample retires at depth 0, with a colour that depends on the
// iteration's specular / diffuse draw: the rule is off.  PtOptions.debug_flags kRetireEveryIteration: off as an A/B switch.
constexpr int kRetireEveryIteration = 1024;
// Slot i of a region (q, k) -> the sub-region (q, k, rho) that holds it and its position there: the inverse of sub_offset /
// sub_chunks.  Residues below rem own quo + 1 chunks each, the others quo; slots behind the last sub-region
// (i >= my_nq * 64) do not exist.  (quo = my_nq / wq0, rem = my_nq % wq0)
struct SubSlot {
  int rho, pos;
};
PT_SCHED SubSlot sub_slot(int quo, int rem, int i) {
  const int c = i >> 6, big = rem * (quo + 1);  // chunks of the residues that own quo + 1
  const int rho = c < big ? c / (quo + 1) : rem + (c - big) / sched_max(quo, 1);
  return SubSlot{rho, i - sub_offset(quo, rem, rho) * 64};
}
// Slot i is a depth-0 retiree slot: it lies in the front of its sub-region, among the `retirees` records k_primary puts there.
PT_SCHED bool retiree_slot(const SubSlot& s, int retirees) { return s.pos < retirees; }

// ── depth-1 records: the iteration-invariant half written once per batch ──────────────────────────────────────────────────
// In a batch that retires once (above) the lanes that SURVIVE depth 0 are the same in every iteration too, so with
// shared_rho(r, k, wq) = r record i of sub-list (q, k, r) belongs to the same pixel for every k.  Of its 40 bytes the origin
// hp + 0.001 * hn is a function of the first hit alone, and the throughput — depth 0 has no roulette — is (1, 1, 1) times the
// hit material's spec or color, whichever the iteration's specular / diffuse draw chose: only the direction, the sample id
// and that one bit differ between iterations.  Such a batch (BatchInfo::split_records) keeps, in the same buffers at the
// same strides,
//   plane 0, slot at                   (direction.xyz, sample id | kind << 31)   per iteration, as before
//   plane 1, slot at - k * seg_cap     (origin.xyz, material index)              once, by the run that holds iteration 0
// and leaves plane 2 alone; k_paths forms the throughput from its material table.  (trace_depth 1: nobody survives; jitter,
// flat lists, a trace per iteration: whole records.)  PtOptions.debug_flags kWholeRecords: off as an A/B switch.
constexpr int kWholeRecords = 4096;
// Where the invariant half of the record at path slot `at` = k * seg_cap + sub_offset(quo, rem, rho) * 64 + i of a queue lives:
// the same slot of iteration 0.
PT_SCHED int invariant_slot(int at, int k, int seg_cap) { return at - k * seg_cap; }
// The per-iteration word's last lane: sample ids k << slot_shift | pl use 31 bits (k < 2^(31 - slot_shift), pt_init), bit 31
// carries what shade_decide decided at depth 0: 1 specular (throughput = spec), 0 diffuse (throughput = color).
PT_SCHED uint32_t pack_kind(int sample_id, bool specular) { return (uint32_t)sample_id | (specular ? 0x80000000u : 0u); }
PT_SCHED int kind_sample_id(uint32_t word) { return (int)(word & 0x7fffffffu); }
PT_SCHED bool kind_specular(uint32_t word) { return (word >> 31) != 0u; }

// ── depth-1 records: the first bounce sampled in k_paths ──────────────────────────────────────────────────────────────────
// In a batch that splits its records everything the depth-0 shading of a surviving pixel does per iteration — the seed, the one
// specular / diffuse draw, the direction sampling — is a pure function of the pixel's first hit and the iteration.  Such a batch
// (BatchInfo::split_records == kFirstBounce) stores ONE whole 40-byte record per surviving pixel and batch, at the slot its record has
// in iteration 0 (invariant_slot), and nothing per iteration:
//   origin      bounce_origin(hit normal, hit point)                      where PathBuf keeps a path's origin
//   hit normal                                                            where it keeps the direction
//   camera direction                                                      where it keeps the throughput
//   tile pixel | material index << slot_shift  (pack_first)               where it keeps the sample id
// k_primary traces a chunk once per batch and publishes the same pair of counts for every iteration; a lane of k_paths that takes
// the record of sub-list (k, rho) decides depth 0 for iteration k itself and samples the first bounce with the lanes that
// survived that round.  It needs the LDS-table search form (the other forms keep the next record in registers; they stay with split
// records), a material index that fits beside the tile pixel, and a K that fits beside the visit number (pack_visit).
// PtOptions.debug_flags kNoFirstBounce: off as an A/B switch.
constexpr int kNoFirstBounce = 8192;
constexpr int kSplitRecords = 1, kFirstBounce = 2;  // BatchInfo::split_records
constexpr int kSearchLdsTables = 0;                  // FormInputs::search_form: pt_lds.h kLdsTables
// The word that waits with a record in a lane's refill slot: the iteration k of its sub-list above the visit number modulo
// 2^kVisitBits.  A path in flight was taken fewer than kVisitRing (pt_lds.h) <= 2^(kVisitBits - 1) visits ago, so the distance
// of two visit numbers is compared modulo the packed width (visit_gap).
constexpr int kVisitBits = 8;
PT_SCHED uint32_t pack_visit(int k, int visit) { return ((uint32_t)k << kVisitBits) | ((uint32_t)visit & ((1u << kVisitBits) - 1u)); }
PT_SCHED int visit_k(uint32_t word) { return (int)(word >> kVisitBits); }
PT_SCHED int visit_number(uint32_t word) { return (int)(word & ((1u << kVisitBits) - 1u)); }  // modulo 2^kVisitBits
PT_SCHED int visit_gap(int visits_now, int visit) { return (visits_now - visit) & ((1 << kVisitBits) - 1); }
PT_SCHED bool visit_k_fits(int K) { return K <= (1 << (31 - kVisitBits)); }
// The record's last word: tile pixel pl < 2^slot_shift below the material index, 31 bits in all.
PT_SCHED int pack_first(int pl, int mat, int slot_shift) { return (mat << slot_shift) | pl; }
PT_SCHED int first_pixel(int word, int slot_shift) { return word & ((1 << slot_shift) - 1); }
PT_SCHED int first_material(int word, int slot_shift) { return (int)((uint32_t)word >> slot_shift); }
PT_SCHED bool first_material_fits(int num_mats, int slot_shift) { return num_mats <= (1 << (31 - slot_shift)); }

// ── depth 0 of a first-bounce batch: traced once per camera ───────────────────────────────────────────────────────────────
// What k_primary leaves behind in a first-bounce batch — the surviving pixels' records at their slots of iteration 0, the depth-0
// retirees' records at the front of the sub-regions of iteration 0, the pair of counts in sub[] — depends on the camera, the scene
// tables, the tile or list and the queue geometry, and on neither the batch's first iteration nor (the counts are published for every
// iteration the regions are provisioned for, RetireBuf::kmax) on how many it holds; k_paths and the gathers only read it.  So the next
// such batch of the same context finds it as it needs it, and the host launches k_primary only when one of those inputs has changed
// (pt_api.cpp run_batch keeps the launch's arguments as the key).  The counter row of depth 0, which the statistics read and re-zero
// after every batch, is written by k_paths in this form.  Every other form's depth 0 has per-iteration output and is traced in every
// batch.  The rule holds for the batches with fixed record slots (the rung behind them in batch_form below): there k_paths' own stores
// into the record regions go to slots the path's list position gives, behind the retirees', in every batch alike.
// PtOptions.debug_flags kPrimaryEveryBatch: in every batch, as an A/B switch.
constexpr int kPrimaryEveryBatch = 65536;

// ── retirement records of a first-bounce batch: fixed slots, gathered as a stream ─────────────────────────────────────────
// In a first-bounce batch record i of sub-list (q, k, rho) is the same pixel for every k (above), and the lane of k_paths that takes
// it knows i.  Such a batch (BatchInfo::fixed_slots) stores the path's retirement record at slot retirees(rho) + i of sub-region
// (q, k, rho) — the range the wave's visit of the sub-list fills anyway, in list order instead of in order of retirement — so slot s of
// region (q, k) holds the same pixel for every k, and the gather (k_collect_stream, pt_output.inc) needs no tile: one thread per slot
// adds its K records in iteration order.  PtOptions.debug_flags kRecordsByVisit: records in order of retirement and the tile gather;
// kTileGather: fixed slots under the tile gather, which places a record by its pixel word wherever it lies.
constexpr int kRecordsByVisit = 16384, kTileGather = 32768;
constexpr int kFixedSlots = 3;  // k_paths' SPLIT argument for such a batch (BatchInfo::split_records stays kFirstBounce: k_primary does not care)
// The record slot, inside its queue's regions, of the path at list position i of sub-list (k, rho).  (quo, rem: sub_offset)
PT_SCHED int fixed_slot(int k, int seg_cap, int quo, int rem, int rho, int retirees, int i) { return k * seg_cap + sub_offset(quo, rem, rho) * 64 + retirees + i; }
// The word that waits with a record in a lane's refill slot, in place of pack_visit: the iteration k above the slot's offset in its
// region, slot - k * seg_cap < seg_cap, in fixed_bits(seg_cap) bits.  The take shifts k out and forms the slot with one multiply-add
// (the whole slot alone would cost the lane a division by seg_cap for k).  (seg_cap >= 64: a multiple of 64)
PT_SCHED int fixed_bits(int seg_cap) { return 32 - __builtin_clz((unsigned)(seg_cap - 1)); }
PT_SCHED uint32_t pack_fixed(int k, int in_region, int bits) { return ((uint32_t)k << bits) | (uint32_t)in_region; }
PT_SCHED int fixed_k(uint32_t word, int bits) { return (int)(word >> bits); }
PT_SCHED int fixed_slot_of(uint32_t word, int bits, int seg_cap) { return (int)(word >> bits) * seg_cap + (int)(word & ((1u << bits) - 1u)); }
PT_SCHED bool fixed_word_fits(int K, int seg_cap) { return K <= (1 << (31 - fixed_bits(seg_cap))); }
// k_paths' SPLIT argument from BatchInfo::split_records and BatchInfo::fixed_slots (BatchForm::split; pt_launch.inc launch_paths).
PT_SCHED int paths_split(int records, bool fixed_slots) { return records == kFirstBounce && fixed_slots ? kFixedSlots : records; }

// ── the form of a batch: the rungs above, each a step from the one before it ──────────────────────────────────────────────
// Host code only: run_batch (pt_api.cpp) decides the form once per batch and copies it into BatchInfo::retire_once, split_records and
// fixed_slots; the kernels and their launch wrappers read those.  (tests/test_sched_form.py)
struct FormInputs {  // (search_form: pt_lds.h Search of the context's tables; seg_cap: RetireBuf::seg_cap)
  int primary_share;
  bool aa_jitter, flat;
  int trace_depth, debug_flags, search_form, num_mats, slot_shift, K, seg_cap;
};
PT_SCHED FormInputs form_inputs(const BatchInfo& b, int debug_flags, int search_form, int num_mats, int seg_cap) {
  return FormInputs{b.primary_share, b.aa_jitter != 0, b.flat != 0, b.trace_depth, debug_flags, search_form, num_mats, b.slot_shift, b.K, seg_cap};
}
struct BatchForm {
  bool shares, retire_once;  // k_primary's shared form; BatchInfo::retire_once
  int records;               // BatchInfo::split_records: 0, kSplitRecords or kFirstBounce
  bool fixed_slots;          // BatchInfo::fixed_slots
  bool primary_once;         // the batch reads the first-hit records an earlier batch of the same camera, tile and plan left
  int split;                 // k_paths' SPLIT argument (paths_split)
};
PT_SCHED BatchForm batch_form(const FormInputs& in) {
  BatchForm f{};
  f.shares = primary_shares(in.primary_share, in.aa_jitter, in.flat);
  const bool invariant = f.shares && in.trace_depth >= 2;  // what leaves depth 0, and how, is a function of the pixel alone
  f.retire_once = invariant && !(in.debug_flags & kRetireEveryIteration);
  const bool splits = invariant && !(in.debug_flags & kWholeRecords);
  const bool first = splits && f.retire_once && !(in.debug_flags & kNoFirstBounce) && in.search_form == kSearchLdsTables &&
                     first_material_fits(in.num_mats, in.slot_shift) && visit_k_fits(in.K);
  f.records = first ? kFirstBounce : splits ? kSplitRecords : 0;
  f.fixed_slots = first && fixed_word_fits(in.K, in.seg_cap) && !(in.debug_flags & kRecordsByVisit);
  f.primary_once = f.fixed_slots && !(in.debug_flags & kPrimaryEveryBatch);
  f.split = paths_split(f.records, f.fixed_slots);
  return f;
}
// Every value of BatchForm::records and of BatchForm::split: what a context's batches can ask of k_primary and k_paths (residency).
constexpr int kRecordForms[] = {0, kSplitRecords, kFirstBounce}, kPathsSplits[] = {0, kSplitRecords, kFirstBounce, kFixedSlots};

// ── the gather of a batch: one plan ───────────────────────────────────────────────────────────────────────────────────────
// PtStats.gather_form of a batch: 0 the tile gather over records in order of retirement, 1 the tile gather over fixed slots (kTileGather,
// and every batch with the convergence metric, whose partial sums keep their partition), 2 the stream.
constexpr int kGatherTile = 0, kGatherTileFixed = 1, kGatherStream = 2;
// The stream gather of a batch inside the NEXT batch's k_paths (PtStats.gather_form 3 while such a batch waits; the last batch of a render
// call is always gathered by k_collect_stream, so a finished call reports 2 and PtStats.inline_gathers counts the others).  k_paths is bound
// by instruction issue and leaves most of the memory system idle, the gather is memory traffic alone, and as separate launches they run
// one after the other: the waves of batch n + 1 therefore add batch n's records to the image in small steps beside their own work
// (pt_kernels.hip k_paths, PREV).  Batch n + 1 stores its records in the other of two record planes; what k_primary writes once per
// camera — the depth-0 retirees' records, sub[] — stays in plane 0 and is only read.  The second plane may not be used in a context with
// the convergence metric, whose batches change form in mid-call.  Noise folds, read-backs and camera moves happen between render calls,
// where nothing waits.  PtOptions.debug_flags kGatherEveryBatch: every batch by k_collect_stream, as an A/B switch.
constexpr int kGatherInline = 3, kGatherEveryBatch = 131072;
// The switches under which no batch of a context takes that form (such a context gets no second plane), and every switch read here.
constexpr int kNoSecondPlane = kGatherEveryBatch | kTileGather | kRecordsByVisit | kNoFirstBounce | kPrimaryEveryBatch;
constexpr int kFormSwitches = kTraceEveryIteration | kRetireEveryIteration | kWholeRecords | kNoSecondPlane;
struct GatherInputs {
  BatchForm form;
  bool metric, waiting;  // the batch carries the convergence metric; the batch before it waits for its gather ...
  int waiting_plane;     // ... with its records in this plane
  bool same_key;         // this batch launches no k_primary (run_batch's PrimaryKey is unchanged)
  bool second_plane;     // the second plane exists and may be used
  int after, debug_flags;  // after: batches of the same render call that follow this one
  bool fused;            // the bounces run in k_paths
};
// The launch that closes a batch: the stream gather with the counter rows' blocks (records in plane 0), or k_count_stats and then
// the stream gather over both planes, the tile gather with or without the metric, or nothing (the gather waits).
enum Closing { kCloseStream, kCloseStatsStreamPlanes, kCloseStatsConv, kCloseStatsTile, kCloseStats };
struct GatherPlan {
  int form;                      // kGatherTile, kGatherTileFixed or kGatherStream
  bool gathers_waiting, defers;  // this batch's k_paths gathers the batch before it; its own gather waits for the next batch's k_paths
  int plane, reported;           // the record plane this batch's k_paths writes; PtStats.gather_form
  Closing closing;
};
// A batch whose gather waits stores its records in plane `after` mod 2, so that the planes alternate along the call and its last batch —
// which never waits, like the only batch of a call — lies in plane 0; a batch that gathers its predecessor takes the plane that one did
// not use (the same thing, unless the chain began in mid-call).
PT_SCHED GatherPlan gather_plan(const GatherInputs& in) {
  GatherPlan p{};
  p.form = !in.form.fixed_slots ? kGatherTile : (in.debug_flags & kTileGather) || in.metric ? kGatherTileFixed : kGatherStream;
  const bool chains = p.form == kGatherStream && in.form.primary_once && in.second_plane && in.fused && !(in.debug_flags & kGatherEveryBatch);
  p.gathers_waiting = chains && in.waiting && in.same_key;
  p.defers = chains && in.after > 0;
  p.plane = p.gathers_waiting ? 1 - in.waiting_plane : p.defers ? in.after & 1 : 0;
  p.reported = p.defers ? kGatherInline : p.form;
  if (p.defers) p.closing = kCloseStats;
  else if (p.form == kGatherStream) p.closing = p.plane == 0 ? kCloseStream : kCloseStatsStreamPlanes;
  else p.closing = in.metric ? kCloseStatsConv : kCloseStatsTile;
  return p;
}

// ── k_paths: falling pieces ───────────────────────────────────────────────────────────────────────────────────────────────
// BatchInfo::paths_pieces: pieces per wave | fewest paths in a piece << 16.
PT_SCHED int pack_paths_pieces(int count, int min_piece) { return count | min_piece << 16; }
PT_SCHED int paths_pieces_count(int word) { return word & 0xffff; }
PT_SCHED int paths_pieces_min(int word) { return word >> 16; }
// A queue's depth-1 ranks [0, total) cut into pieces for its wq waves.  Piece p belongs to level p / wq; a level has wq pieces
// of one size, ps0 at level 0 and (1 - 1 / P) of the previous level's after that, never below ps_min (P = pieces_per_wave).
// Pieces 0 .. wq - 1 are the waves' own; the later ones are handed out by the queue's counter, which exists only when
// level 0 does not cover the queue.
struct PieceRange {
  int start, end;
  bool some;  // false: no such piece (and start == end == total)
};
struct PiecePlan {
  int total, wq, pieces_per_wave, ps_min, ps0;
  PT_SCHED bool needs_counter() const { return ps0 * wq < total; }
  PT_SCHED PieceRange piece_range(int nextp) const {  // nextp < 0: none
    int start = total, sz = ps0;
    if (nextp >= 0) {
      start = 0;
      int level = nextp / wq;
      const int idx = nextp - level * wq;
      for (; level > 0 && start < total; --level) start += wq * sz, sz = sched_max(sz - sz / pieces_per_wave, ps_min);
      start += idx * sz;
    }
    return start < total ? PieceRange{start, sched_min(start + sz, total), true} : PieceRange{total, total, false};
  }
};
// (pieces only with a deal table behind the counters and with k_paths' chunk sums, i.e. at most 4096 sub-lists)
PT_SCHED PiecePlan piece_plan(int total, int wq, int paths_pieces, bool deal_present, bool chunk_sums) {
  PiecePlan p;
  p.total = total, p.wq = wq;
  p.pieces_per_wave = deal_present && chunk_sums && paths_pieces_count(paths_pieces) > 1 ? paths_pieces_count(paths_pieces) : 1;
  p.ps_min = paths_pieces_min(paths_pieces);
  p.ps0 = sched_max((total + wq * p.pieces_per_wave - 1) / (wq * p.pieces_per_wave), p.ps_min);
  return p;
}

}  // namespace ptk
