// Prints the first-bounce rule of csrc/pt_sched.h — which batches store one record per surviving pixel and leave the first
// bounce to k_paths, the record's last word, and the word that waits beside a record in a refill slot — over a sweep
// (tests/test_sched_first_bounce.py compiles this with the system compiler, runs it and checks the output by enumeration).
// Output: one line per case, `name key=value ...`.
#include <cstdint>
#include <cstdio>

#include "pt_lds.h"
#include "pt_sched.h"

using namespace ptk;

int main() {
  printf("consts bit=%d split=%d first=%d visit_bits=%d visit_ring=%d\n", kNoFirstBounce, kSplitRecords, kFirstBounce, kVisitBits, kVisitRing);
  // rule: the predicate over its conditions, as a function and on a BatchInfo, and the record form the host stores
  for (int share : {-1, 1, 2, 64})
    for (int aa = 0; aa < 2; ++aa)
      for (int flat = 0; flat < 2; ++flat)
        for (int depth : {1, 2, 8})
          for (int flags : {0, 16, 128, 1024, 4096, 8192, 8192 | 4096, 8192 | 1024})
            for (int form : {0, 1, 2})
              for (int mats : {1, 8, 9})      // slot_shift 28 below: 2^(31 - 28) = 8 material indices fit
                for (int K : {1, 25, 1 << (31 - kVisitBits), (1 << (31 - kVisitBits)) + 1}) {
                  BatchInfo b{};
                  b.primary_share = share, b.aa_jitter = aa, b.flat = flat, b.trace_depth = depth, b.slot_shift = 28, b.K = K;
                  printf("rule share=%d aa=%d flat=%d depth=%d flags=%d form=%d mats=%d K=%d shift=%d first=%d first_b=%d record_form=%d split=%d once=%d\n", share, aa, flat,
                         depth, flags, form, mats, K, b.slot_shift, (int)first_bounces(share, aa != 0, flat != 0, depth, flags, form, mats, b.slot_shift, K),
                         (int)first_bounces(b, flags, form, mats), record_form(b, flags, form, mats), (int)splits_records(b, flags), (int)retires_once(b, flags));
                }
  // fits: the two fallbacks on their own, at every slot_shift
  for (int shift = 1; shift <= 30; ++shift)
    for (int mats : {1, (1 << (31 - shift)) - 1, 1 << (31 - shift), (1 << (31 - shift)) + 1})
      if (mats > 0) printf("fits shift=%d mats=%d ok=%d\n", shift, mats, (int)first_material_fits(mats, shift));
  for (int K : {1, 64, 65, 256, (1 << (31 - kVisitBits)) - 1, 1 << (31 - kVisitBits), (1 << (31 - kVisitBits)) + 1}) printf("kfits K=%d ok=%d\n", K, (int)visit_k_fits(K));
  // first: the record's last word for the smallest and the largest pixel and material of every slot_shift
  for (int shift = 1; shift <= 30; ++shift)
    for (int pl : {0, (1 << shift) - 1})
      for (int mat : {0, 1, (1 << (31 - shift)) - 1}) {
        const int w = pack_first(pl, mat, shift);
        printf("first shift=%d pl=%d mat=%d word=%d out_pl=%d out_mat=%d\n", shift, pl, mat, w, first_pixel(w, shift), first_material(w, shift));
      }
  // visit: the waiting word of (k, visit number) — the visit number counts on without bound, the word keeps it modulo 2^kVisitBits
  for (int k : {0, 1, 63, 64, 255, (1 << (31 - kVisitBits)) - 1})
    for (int visit : {0, 1, 63, 64, 255, 256, 257, 100000, 0x7fffffff}) {
      const uint32_t w = pack_visit(k, visit);
      printf("visit k=%d visit=%d word=%u out_k=%d out_visit=%d\n", k, visit, (unsigned)w, visit_k(w), visit_number(w));
    }
  // gap: the lap comparison across a wrap of the packed width — a path taken at visit `then`, the cursor at visit `now`
  for (int then : {0, 1, 200, 255, 256, 511, 65535, 65536, 1000000})
    for (int ahead = 0; ahead <= kVisitRing; ++ahead) {
      const int now = then + ahead;
      printf("gap then=%d now=%d ahead=%d gap=%d\n", then, now, ahead, visit_gap(now, visit_number(pack_visit(0, then))));
    }
  BatchInfo zero{};
  printf("fresh split_records=%d\n", (int)zero.split_records);
  return 0;
}
