// Prints csrc/pt_sched.h's work distribution for a sweep of (N, Q, wq0, K, pieces) (tests/test_sched.py compiles this with
// the system compiler, runs it and checks the output by enumeration).  Output: one header line per case (`name key=value
// ...`), followed — where a case enumerates something — by lines of plain numbers whose meaning the header's name fixes.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pt_sched.h"

using namespace ptk;

static const int kN[] = {1, 63, 64, 65, 700, 4097, 259200, 2073600};
static const int kQ[] = {1, 4, 32, 256, 1024};
static const int kWq[] = {1, 2, 3, 6, 20, 24};
static const int kK[] = {1, 2, 3, 25, 195, 256};

static ptd::Queues queues(int Q, int W) {
  ptd::Queues qs{};
  qs.Q = Q, qs.W = W, qs.cnt_stride = 16;
  return qs;
}

static void put_deal_maps() {
  for (int Q : kQ) {
    const DealMap m = deal_map(queues(Q, Q));
    printf("dealmap Q=%d first0=%d firstQ=%d made_for=%d time0=%d timeL=%d strand=%d piece0=%d pieceL=%d rays0=%d raysL=%d words=%d\n", Q, m.first(0),
           m.first(Q), m.made_for(), m.time(0), m.time(Q - 1), m.strand_counter(), m.piece_counter(0), m.piece_counter(Q - 1), m.rays(0), m.rays(Q - 1),
           m.words());
  }
}

// queue geometry: per (N, Q) one `q` line per queue — q my_nq my_pixels, slot_pixel of the queue's first and last slots of
// its first and last chunks (4 numbers, -1 without chunks), then chunk_pixel of every chunk jj; per (N, Q, wq0) one `s` line
// per queue with chunks (and the first without) — q g0 g1, then sub_chunks, sub_offset per residue.
static void put_geometry() {
  for (int N : kN)
    for (int Q : kQ) {
      BatchInfo b{};
      b.N = N;
      const ptd::Queues qs = queues(Q, Q);
      printf("geo N=%d Q=%d\n", N, Q);
      for (int q = 0; q < Q; ++q) {
        const QueueShare sh = queue_share(b, qs, q);
        const int last = sh.my_nq * 64 - 1;
        printf("q %d %d %d %d %d %d %d", q, sh.my_nq, sh.my_pixels, sh.my_nq ? slot_pixel(q, 0, Q) : -1, sh.my_nq ? slot_pixel(q, 63, Q) : -1,
               sh.my_nq ? slot_pixel(q, last - 63, Q) : -1, sh.my_nq ? slot_pixel(q, last, Q) : -1);
        for (int jj = 0; jj < sh.my_nq; ++jj) printf(" %d", chunk_pixel(q, jj, Q));
        printf("\n");
      }
      for (int wq0 : kWq) {
        printf("sub N=%d Q=%d wq0=%d\n", N, Q, wq0);
        bool empty_seen = false;
        for (int q = 0; q < Q; ++q) {
          const QueueShare sh = queue_share(b, qs, q);
          if (sh.my_nq == 0 && empty_seen) continue;
          empty_seen |= sh.my_nq == 0;
          const Gap g = region_gap(sh, wq0);
          printf("s %d %d %d", q, g.g0, g.g1);
          const int quo = sh.my_nq / wq0, rem = sh.my_nq % wq0;
          for (int rho = 0; rho < wq0; ++rho) printf(" %d %d", sub_chunks(quo, rem, rho), sub_offset(quo, rem, rho));
          printf("\n");
        }
      }
      for (int K : kK) {
        const QueuePlan p = queue_plan(N, Q, K);
        printf("plan N=%d Q=%d K=%d nq=%d chunks_per_queue=%d seg_cap=%d cap=%d\n", N, Q, K, p.nq, chunks_per_queue(N, Q), p.seg_cap, p.cap);
      }
    }
  for (int Q : kQ)
    for (int wq0 : kWq) {
      const int W = Q * wq0;
      printf("waves Q=%d W=%d sub_stride=%d\n", Q, W, (int)sub_stride(W, Q));
      for (int w = 0; w < W; ++w) {
        const WaveSlot s = wave_slot(w, Q, W);
        printf("%d %d %d ", s.q, s.r, s.wq);
      }
      printf("\n");
    }
  for (int Q : kQ)
    for (int stride : {1, 16})
      for (int d : {0, 1, 7, 64}) {
        ptd::Queues qs = queues(Q, Q);
        qs.cnt_stride = stride;
        printf("cnt Q=%d stride=%d d=%d first=%lld last=%lld\n", Q, stride, d, (long long)cnt_index(qs, d, 0), (long long)cnt_index(qs, d, Q - 1));
      }
}

// strands: `rho` tables per wq (strand_rho, strand_rho_before for r < wq, k < 256), then per case the plan and p q r wq k0 k1
// of every strand index 0 .. W * pieces - 1.  The full product for Q <= 4; a diagonal of (wq0, K, pieces) for the larger Q.
static void put_strands() {
  for (int wq : kWq) {
    printf("rho wq=%d K=256\n", wq);
    for (int r = 0; r < wq; ++r)
      for (int k = 0; k < 256; ++k) printf("%d %d ", strand_rho(r, k, wq), strand_rho_before(r, k, wq));
    printf("\n");
  }
  const int kPieces[] = {0, 1, 2, 3, 4, 7};
  const int diagonal[][3] = {{1, 1, 0}, {2, 2, 7}, {3, 3, 2}, {6, 25, 4}, {20, 195, 3}, {24, 25, 2}, {2, 256, 1}};
  for (int Q : kQ)
    for (int wq0 : kWq)
      for (int K : kK)
        for (int pp : kPieces) {
          bool wanted = Q <= 4;
          for (const auto& d : diagonal) wanted |= d[0] == wq0 && d[1] == K && d[2] == pp;
          if (!wanted) continue;
          const int W = Q * wq0;
          // (deal table, flat form): pieces only with the first and without the second; the other combinations on the diagonal
          for (int form = 0; form < (Q == 4 ? 4 : 1); ++form) {
            const bool deal = !(form & 1), flat = form & 2;
            const StrandPlan p = strand_plan(K, pp, deal, flat);
            printf("strands Q=%d W=%d K=%d pp=%d deal=%d flat=%d kp=%d pieces=%d\n", Q, W, K, pp, deal, flat, p.kp, p.pieces);
            for (int s = 0; s < W * p.pieces; ++s) {
              const Strand st = strand_of(s, p, K, Q, W);
              printf("%d %d %d %d %d %d ", st.piece, st.q, st.r, st.wq, st.k0, st.k1);
            }
            printf("\n");
          }
        }
  for (int K : kK)
    for (int nq : {0, 1, 2, 13, 127, 128, 32400})
      for (int wq0 : {0, 1, 2, 3, 6, 20, 24}) printf("auto_pieces K=%d nq=%d wq0=%d pieces=%d\n", K, nq, wq0, auto_primary_pieces(K, nq, wq0));
}

// paths pieces: per case the plan, then start end some of nextp = -1, 0, 1, ... up to 3 * wq + 3 beyond the first empty one.
static void put_paths_pieces() {
  const int totals[] = {0, 1, 2, 63, 64, 65, 127, 1000, 4097, 50000};
  for (int total : totals)
    for (int wq : {1, 2, 3, 6, 24})
      for (int count : {1, 2, 3, 4, 8})
        for (int min_piece : {1, 3, 64})
          for (int form = 0; form < (total == 1000 ? 4 : 1); ++form) {
            const bool deal = !(form & 1), sums = !(form & 2);
            const int word = pack_paths_pieces(count, min_piece);
            const PiecePlan p = piece_plan(total, wq, word, deal, sums);
            printf("pieces total=%d wq=%d count=%d min_piece=%d deal=%d sums=%d word=%d ucount=%d umin=%d ppw=%d ps_min=%d ps0=%d needs_counter=%d\n", total, wq,
                   count, min_piece, deal, sums, word, paths_pieces_count(word), paths_pieces_min(word), p.pieces_per_wave, p.ps_min, p.ps0,
                   p.needs_counter() ? 1 : 0);
            int after_empty = 0;
            for (int nextp = -1; after_empty < 3 * wq + 3; ++nextp) {
              const PieceRange r = p.piece_range(nextp);
              printf("%d %d %d ", r.start, r.end, r.some ? 1 : 0);
              if (nextp >= 0 && !r.some) ++after_empty;
            }
            printf("\n");
          }
}

// the deal: per (Q, wq, work vector) the work, then dealt_first(q) for q = 0 .. Q from the prefix sums, and the
// close-together predicate with the same vector as rays.
static void put_deal() {
  uint64_t rng = 0x9e3779b97f4a7c15ull;
  auto next = [&rng]() {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng >> 33);
  };
  for (int Q : kQ)
    for (int wq : kWq) {
      const int W = Q * wq;
      for (int kind = 0; kind < 9; ++kind) {
        std::vector<int> work(Q);
        for (int q = 0; q < Q; ++q) {
          switch (kind) {
            case 0: work[q] = 1 + (int)(next() % 100000); break;               // random
            case 1: work[q] = 1000 + (int)(next() % 60); break;                // random, close together
            case 2: work[q] = q == 0 ? 12345 : 0; break;                       // all in the first queue
            case 3: work[q] = q == Q - 1 ? 12345 : 0; break;                   // all in the last
            case 4: work[q] = q == Q / 2 ? 1 : 0; break;                       // one unit in the middle
            case 5: work[q] = q % 2 ? 0 : 1 + (int)(next() % 1000); break;     // every other queue idle
            case 6: work[q] = 0x7fffffff; break;                               // the largest a counter holds
            case 7: work[q] = 7; break;                                        // equal
            default: work[q] = q < Q - 1 && next() % 3 ? 0 : 0x3ffff * 24; break;  // mostly idle, the rest saturated ticks
          }
        }
        unsigned long long total = 0;
        int heaviest = 0;
        for (int w : work) total += (unsigned long long)w, heaviest = w > heaviest ? w : heaviest;
        printf("deal Q=%d W=%d kind=%d close=%d\n", Q, W, kind, queues_close_together(heaviest, total, W, Q) ? 1 : 0);
        for (int w : work) printf("%d ", w);
        printf("\n");
        unsigned long long before = 0;
        for (int q = 0; q <= Q; ++q) {
          printf("%d ", dealt_first(q, W, Q, before, total));
          if (q < Q) before += (unsigned long long)work[q];
        }
        printf("\n");
      }
    }
}

int main() {
  put_deal_maps();
  put_geometry();
  put_strands();
  put_paths_pieces();
  put_deal();
  return 0;
}
