// Prints the slot map behind the retire-once rule of csrc/pt_sched.h — from a region's slot to its sub-region and position there —
// over a sweep (tests/test_sched_retire_once.py compiles this with the system compiler, runs it and checks the output by
// enumeration; which batches retire once: tests/sched_form_driver.cpp).  Output: one header line per case (`name key=value ...`) followed
// by lines of plain numbers.
#include <cstdint>
#include <cstdio>

#include "pt_sched.h"

using namespace ptk;

// Retirees of sub-region rho for the sweep's `fill`: 0 none, 1 every pixel it has, 2 .. some number in between (a hash of rho).
static int retirees_of(int fill, int rho, int pixels) {
  if (fill == 0) return 0;
  if (fill == 1) return pixels;
  return (int)(((uint32_t)rho * 2654435761u + (uint32_t)fill * 40503u) % (uint32_t)(pixels + 1));
}

// slots: per case (tile of N pixels, Q queues, wq0 residues, K iterations, queue q) line 1: rho pos of every slot of a region;
// line 2, per fill 0 .. 3: the retirees of every residue, then the retiree bit of every slot.
static void put_slots() {
  for (int N : {1, 63, 64, 65, 700, 4097, 23919})
    for (int Q : {1, 4, 32})
      for (int wq0 : {1, 2, 3, 6, 20, 24})
        for (int K : {1, 25}) {
          BatchInfo b{};
          b.N = N, b.K = K;
          ptd::Queues qs{};
          qs.Q = Q, qs.W = Q * wq0, qs.cnt_stride = 16;
          const QueuePlan plan = queue_plan(N, Q, K);
          for (int q = 0; q < Q; ++q) {
            if (Q > 4 && q != 0 && q != Q - 1 && q != ((N + 63) / 64 - 1) % Q) continue;  // the larger Q: the first, the last and the partial chunk's queue
            const QueueShare sh = queue_share(b, qs, q);
            const int quo = sh.my_nq / wq0, rem = sh.my_nq % wq0, n = sh.my_nq * 64;
            const Gap g = region_gap(sh, wq0);
            printf("slots N=%d Q=%d wq0=%d K=%d q=%d my_nq=%d my_pixels=%d seg_cap=%d cap=%d g0=%d g1=%d\n", N, Q, wq0, K, q, sh.my_nq, sh.my_pixels, plan.seg_cap, plan.cap, g.g0, g.g1);
            for (int i = 0; i < n; ++i) {
              const SubSlot s = sub_slot(quo, rem, i);
              printf("%d %d ", s.rho, s.pos);
            }
            printf("\n");
            for (int fill = 0; fill < 4; ++fill) {
              for (int rho = 0; rho < wq0; ++rho) {
                const int first = sub_offset(quo, rem, rho) * 64, slots = sub_chunks(quo, rem, rho) * 64;
                const int pixels = slots - (slots > 0 && g.g1 == first + slots ? g.g1 - g.g0 : 0);  // the sub-region with the tile's partial last chunk has fewer
                printf("%d ", retirees_of(fill, rho, pixels));
              }
              for (int i = 0; i < n; ++i) {
                const SubSlot s = sub_slot(quo, rem, i);
                const int first = sub_offset(quo, rem, s.rho) * 64, slots = sub_chunks(quo, rem, s.rho) * 64;
                const int pixels = slots - (slots > 0 && g.g1 == first + slots ? g.g1 - g.g0 : 0);
                printf("%d ", (int)retiree_slot(s, retirees_of(fill, s.rho, pixels)));
              }
            }
            printf("\n");
          }
        }
}

int main() {
  put_slots();
  return 0;
}
