// Prints the rule of csrc/pt_sched.h for tracing depth 0 once per camera — primary_once beside first_bounces and fixed_slots, as a
// function and on a BatchInfo — over a sweep of its conditions (tests/test_sched_primary_once.py compiles this with the system
// compiler, runs it and checks the output by enumeration).  Output: one line per case, `name key=value ...`.
#include <cstdint>
#include <cstdio>

#include "pt_sched.h"

using namespace ptk;

int main() {
  printf("consts every_batch=%d by_visit=%d no_first=%d whole=%d every_iteration=%d tile=%d\n", kPrimaryEveryBatch, kRecordsByVisit, kNoFirstBounce, kWholeRecords,
         kRetireEveryIteration, kTileGather);
  for (int share : {1, 64})
    for (int aa = 0; aa < 2; ++aa)
      for (int flat = 0; flat < 2; ++flat)
        for (int depth : {1, 2, 8})
          for (int flags : {0, 16, 65536, 65536 | 16, 8192, 4096, 1024, 16384, 32768, 65536 | 32768, 65536 | 16384, 128})
            for (int form : {0, 1, 2})
              for (int mats : {8, 9})  // slot_shift 28 below: 2^(31 - 28) = 8 material indices fit
                for (int K : {1, 3, 25, 1 << 18, (1 << 18) + 1}) {  // seg_cap 8128 below: 13 bits, 2^18 iterations fit beside the slot
                  BatchInfo b{};
                  b.primary_share = share, b.aa_jitter = aa, b.flat = flat, b.trace_depth = depth, b.slot_shift = 28, b.K = K;
                  const int seg_cap = 8128;
                  printf("rule share=%d aa=%d flat=%d depth=%d flags=%d form=%d mats=%d K=%d seg_cap=%d first=%d fixed=%d once=%d once_b=%d\n", share, aa, flat, depth, flags, form,
                         mats, K, seg_cap, (int)first_bounces(b, flags, form, mats), (int)fixed_slots(b, flags, form, mats, seg_cap),
                         (int)primary_once(share, aa != 0, flat != 0, depth, flags, form, mats, b.slot_shift, K, seg_cap), (int)primary_once(b, flags, form, mats, seg_cap));
                }
  // a shorter batch of the same plan: the rule that holds for the plan's K holds for every batch length below it
  for (int seg_cap : {64, 8128, 1 << 20})
    for (int K : {1, 2, 25, 256, 1 << 10, 1 << 12})
      for (int kb : {1, K / 2 > 0 ? K / 2 : 1, K})
        printf("shorter seg_cap=%d K=%d kb=%d once_K=%d once_kb=%d\n", seg_cap, K, kb, (int)primary_once(64, false, false, 8, 0, 0, 5, 21, K, seg_cap),
               (int)primary_once(64, false, false, 8, 0, 0, 5, 21, kb, seg_cap));
  return 0;
}
