// Prints the layout behind the fixed-slot rule of csrc/pt_sched.h — the record slot of the path at list position i of sub-list (k, rho)
// and the word that waits beside a record in a refill slot — over a sweep (tests/test_sched_fixed_slots.py compiles this with the system
// compiler, runs it and checks the output by enumeration; which batches store their records that way: tests/sched_form_driver.cpp).
// Output: one header line per case (`name key=value ...`), for `slots` followed by lines of plain numbers.
#include <cstdint>
#include <cstdio>

#include "pt_sched.h"

using namespace ptk;

// Depth-0 retirees of sub-region rho out of its `pixels` for the sweep's `fill`: 0 none, 1 all but one pixel, 2 .. a hash of rho.
static int retirees_of(int fill, int rho, int pixels) {
  if (fill == 0 || pixels == 0) return 0;
  if (fill == 1) return pixels - 1;
  return (int)(((uint32_t)rho * 2654435761u + (uint32_t)fill * 40503u) % (uint32_t)(pixels + 1));
}

// slots: per case (tile of N pixels, Q queues, wq0 residues, K iterations, queue q, fill) a header, then one line per residue rho:
// `rho first slots retirees survivors` followed by, for every iteration k and list position i, the record slot and the waiting
// word's round trip (k out, slot out).
static void put_slots() {
  for (int N : {40, 63, 64, 65, 700, 5917, 23919})
    for (int Q : {1, 4, 256})
      for (int wq0 : {1, 3, 20})
        for (int K : {1, 3, 25, 65}) {
          BatchInfo b{};
          b.N = N, b.K = K;
          ptd::Queues qs{};
          qs.Q = Q, qs.W = Q * wq0, qs.cnt_stride = 16;
          const QueuePlan plan = queue_plan(N, Q, K);
          const int bits = fixed_bits(plan.seg_cap);
          for (int q = 0; q < Q; ++q) {
            if (Q > 4 && q != 0 && q != Q - 1 && q != ((N + 63) / 64 - 1) % Q) continue;  // the larger Q: the first, the last and the partial chunk's queue
            const QueueShare sh = queue_share(b, qs, q);
            if (sh.my_nq == 0 || (int64_t)sh.my_nq * 64 * K > 20000) continue;  // (the long batches on the smaller regions only: the output stays some megabytes)
            const int quo = sh.my_nq / wq0, rem = sh.my_nq % wq0;
            const Gap g = region_gap(sh, wq0);
            for (int fill = 0; fill < 3; ++fill) {
              printf("slots N=%d Q=%d wq0=%d K=%d q=%d fill=%d my_nq=%d seg_cap=%d bits=%d g0=%d g1=%d fits=%d\n", N, Q, wq0, K, q, fill, sh.my_nq, plan.seg_cap, bits, g.g0,
                     g.g1, (int)fixed_word_fits(K, plan.seg_cap));
              for (int rho = 0; rho < wq0; ++rho) {
                const int first = sub_offset(quo, rem, rho) * 64, slots = sub_chunks(quo, rem, rho) * 64;
                const int pixels = slots - (slots > 0 && g.g1 == first + slots ? g.g1 - g.g0 : 0);  // the sub-region with the tile's partial last chunk has fewer
                const int retirees = retirees_of(fill, rho, pixels), survivors = pixels - retirees;
                printf("%d %d %d %d %d", rho, first, slots, retirees, survivors);
                for (int k = 0; k < K; ++k)
                  for (int i = 0; i < survivors; ++i) {
                    const int slot = fixed_slot(k, plan.seg_cap, quo, rem, rho, retirees, i);
                    const uint32_t w = pack_fixed(k, invariant_slot(slot, k, plan.seg_cap), bits);
                    printf(" %d %d %d", slot, fixed_k(w, bits), fixed_slot_of(w, bits, plan.seg_cap));
                  }
                printf("\n");
              }
            }
          }
        }
}

int main() {
  put_slots();
  // word: the largest k and offset of every region size
  for (int seg_cap : {64, 128, 192, 8128, 8192, 8256, 1 << 20, (1 << 20) + 64, 1 << 30}) {
    const int bits = fixed_bits(seg_cap), kmax = 1 << (31 - bits);
    for (int k : {0, 1, kmax - 1})
      for (int off : {0, 1, seg_cap - 1}) {
        const uint32_t w = pack_fixed(k, off, bits);
        printf("word seg_cap=%d bits=%d k=%d off=%d word=%u out_k=%d out_slot=%lld\n", seg_cap, bits, k, off, (unsigned)w, fixed_k(w, bits),
               (long long)fixed_k(w, bits) * seg_cap + (long long)(w & ((1u << bits) - 1u)));
      }
    for (int K : {1, kmax - 1, kmax, kmax + 1}) printf("kfits seg_cap=%d bits=%d K=%d ok=%d\n", seg_cap, bits, K, (int)fixed_word_fits(K, seg_cap));
  }
  return 0;
}
