// Prints the words behind the first-bounce rule of csrc/pt_sched.h — the record's last word, and the word that waits beside a
// record in a refill slot — over a sweep (tests/test_sched_first_bounce.py compiles this with the system compiler, runs it and
// checks the output by enumeration; which batches leave the first bounce to k_paths: tests/sched_form_driver.cpp).
// Output: one line per case, `name key=value ...`.
#include <cstdint>
#include <cstdio>

#include "pt_lds.h"
#include "pt_sched.h"

using namespace ptk;

int main() {
  printf("consts visit_bits=%d visit_ring=%d\n", kVisitBits, kVisitRing);
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
  return 0;
}
