// Prints the layout behind the split-record rule of csrc/pt_sched.h — where the invariant half of a depth-1 record lives, and the
// specular bit beside the sample id — over a sweep (tests/test_sched_split_records.py compiles this with the system compiler, runs
// it and checks the output by enumeration; which batches split their records: tests/sched_form_driver.cpp).  Output: one header line per case (`name key=value ...`)
// followed by lines of plain numbers.
#include <cstdint>
#include <cstdio>

#include "pt_sched.h"

using namespace ptk;

// index: per case (tile of N pixels, Q queues, wq0 residues, K iterations, queue q) and iteration k one line: for every residue r
// and every slot i of sub-list (q, k, r), in that order, the path slot `at` and its invariant slot.  The tile / Q / wq0 / K sweep is
// that of sched_retire_once_driver.cpp.
static void put_index() {
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
            const int quo = sh.my_nq / wq0, rem = sh.my_nq % wq0;
            for (int k : {0, 1, K - 1}) {
              if (k >= K || (k == 1 && K - 1 == 1)) continue;
              printf("index N=%d Q=%d wq0=%d K=%d q=%d k=%d my_nq=%d seg_cap=%d cap=%d\n", N, Q, wq0, K, q, k, sh.my_nq, plan.seg_cap, plan.cap);
              for (int r = 0; r < wq0; ++r) {
                const int first = sub_offset(quo, rem, shared_rho(r, k, wq0)) * 64, slots = sub_chunks(quo, rem, shared_rho(r, k, wq0)) * 64;
                for (int i = 0; i < slots; ++i) {
                  const int at = k * plan.seg_cap + first + i;
                  printf("%d %d ", at, invariant_slot(at, k, plan.seg_cap));
                }
              }
              printf("\n");
              if (K == 1) break;
            }
          }
        }
}

int main() {
  put_index();
  // kind: the word of (k, pl, specular) for the smallest and the largest iteration a batch can hold (pt_init: at most 256 iterations,
  // and k < 2^(31 - slot_shift)) and the smallest and the largest tile pixel, and what comes back out of it
  for (int shift = 1; shift <= 30; ++shift) {
    const int kmax = ((31 - shift) < 8 ? (1 << (31 - shift)) : 256) - 1;
    for (int k : {0, kmax})
      for (int pl : {0, (1 << shift) - 1})
        for (int spec = 0; spec < 2; ++spec) {
          const int id = (k << shift) | pl;
          const uint32_t w = pack_kind(id, spec != 0);
          printf("kind shift=%d k=%d pl=%d spec=%d id=%d word=%u out_id=%d out_spec=%d\n", shift, k, pl, spec, id, (unsigned)w, kind_sample_id(w), (int)kind_specular(w));
        }
  }
  return 0;
}
