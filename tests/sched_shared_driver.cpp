// Prints the shared form of k_primary's schedule (csrc/pt_sched.h: one trace per chunk and run of iterations) for the sweep of
// tests/sched_driver.cpp plus the run caps (tests/test_sched_shared.py compiles this with the system compiler, runs it and
// checks the output by enumeration).  Output: one header line per case (`name key=value ...`) followed by lines of plain numbers.
#include <cstdint>
#include <cstdio>

#include "pt_sched.h"

using namespace ptk;

static const int kQ[] = {1, 4, 32, 256, 1024};
static const int kWq[] = {1, 2, 3, 6, 20, 24};
static const int kK[] = {1, 2, 3, 25, 195, 256};
static const int kPieces[] = {0, 1, 2, 3, 4, 7};
static const int kShare[] = {1, 2, 8, 64};  // BatchInfo::primary_share; 1 is the per-iteration form's value, swept as a cap all the same

// shared: per case the plan; line 1: piece q r wq k0 k1 of every strand index 0 .. W * pieces - 1; line 2: strand s0 s1 of
// every sub-run, in the order the kernel walks them.  The full product for Q <= 4; a diagonal for the larger Q.
static void put_runs() {
  const int diagonal[][3] = {{1, 1, 0}, {2, 2, 7}, {3, 3, 2}, {6, 25, 4}, {20, 195, 3}, {24, 25, 2}, {2, 256, 1}};
  for (int Q : kQ)
    for (int wq0 : kWq)
      for (int K : kK)
        for (int pp : kPieces) {
          bool wanted = Q <= 4;
          for (const auto& d : diagonal) wanted |= d[0] == wq0 && d[1] == K && d[2] == pp;
          if (!wanted) continue;
          const int W = Q * wq0;
          for (int share : kShare) {
            const StrandPlan p = strand_plan(K, pp, true, false);
            const int cap = shared_run_cap(share);
            printf("shared Q=%d W=%d K=%d pp=%d share=%d cap=%d kp=%d pieces=%d max=%d\n", Q, W, K, pp, share, cap, p.kp, p.pieces, kShareMax);
            for (int s = 0; s < W * p.pieces; ++s) {
              const Strand st = strand_of(s, p, K, Q, W);
              printf("%d %d %d %d %d %d ", st.piece, st.q, st.r, st.wq, st.k0, st.k1);
            }
            printf("\n");
            for (int s = 0; s < W * p.pieces; ++s) {
              const Strand st = strand_of(s, p, K, Q, W);
              for (int i = 0, n = shared_runs(st.k0, st.k1, cap); i < n; ++i) {
                const Run r = shared_run(st.k0, st.k1, cap, i);
                printf("%d %d %d ", s, r.k0, r.k1);
              }
            }
            printf("\n");
          }
        }
}

// walk: the kernel's loop nest itself — strand, sub-run, chunk jj of the strand's residue, iteration k of the sub-run — one
// `q k rho jj` per group appended to sub-list (q, k, rho), in that order.
static void put_walks() {
  for (int N : {1, 63, 64, 65, 700, 4097})
    for (int Q : {1, 4})
      for (int wq : {1, 2, 3, 6})
        for (int K : {1, 3, 25})
          for (int pp : {0, 2, 7})
            for (int share : kShare) {
              const int W = Q * wq, cap = shared_run_cap(share);
              BatchInfo b{};
              b.N = N, b.K = K;
              ptd::Queues qs{};
              qs.Q = Q, qs.W = W, qs.cnt_stride = 16;
              const StrandPlan p = strand_plan(K, pp, true, false);
              printf("walk N=%d Q=%d wq=%d K=%d pp=%d share=%d\n", N, Q, wq, K, pp, share);
              for (int s = 0; s < W * p.pieces; ++s) {
                const Strand st = strand_of(s, p, K, Q, W);
                const QueueShare sh = queue_share(b, qs, st.q);
                for (int i = 0, n = shared_runs(st.k0, st.k1, cap); i < n; ++i) {
                  const Run r = shared_run(st.k0, st.k1, cap, i);
                  for (int jj = shared_rho(st.r, r.k0, st.wq); jj < sh.my_nq; jj += st.wq)
                    for (int k = r.k0; k < r.k1; ++k) printf("%d %d %d %d ", st.q, k, shared_rho(st.r, k, st.wq), jj);
                }
              }
              printf("\n");
            }
}

int main() {
  put_runs();
  put_walks();
  for (int K : kK)
    for (int nq : {0, 1, 2, 13, 127, 128, 32400})
      for (int wq0 : {0, 1, 2, 3, 6, 20, 24}) printf("auto_shared K=%d nq=%d wq0=%d pieces=%d\n", K, nq, wq0, auto_shared_pieces(K, nq, wq0));
  for (int share : {-1, 0, 1, 2, 25, 64, 65, 1000})
    for (int aa = 0; aa < 2; ++aa)
      for (int flat = 0; flat < 2; ++flat) printf("form share=%d aa=%d flat=%d shares=%d cap=%d\n", share, aa, flat, (int)primary_shares(share, aa, flat), shared_run_cap(share));
  return 0;
}
