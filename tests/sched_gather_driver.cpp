// Steps the gather plan of csrc/pt_sched.h through render calls of 1 to 6 batches, feeding each batch's plan in as the next batch's
// waiting state the way run_batch does, for tests/test_sched_gather.py (which compiles this with the system compiler, runs it and
// checks the output by enumeration).  Output: a header line, then one line of plain numbers per batch.
#include <cstdio>

#include "pt_sched.h"

using namespace ptk;

int main() {
  printf("cols=chain,n,i,after,second_plane,metric,flags,fused,same_key,fixed,once,waiting,waiting_plane,form,gathers_waiting,defers,plane,reported,closing\n");
  printf("closings=%d,%d,%d,%d,%d\n", (int)kCloseStream, (int)kCloseStatsStreamPlanes, (int)kCloseStatsConv, (int)kCloseStatsTile, (int)kCloseStats);
  const int switches[4] = {kGatherEveryBatch, kTileGather, kRecordsByVisit, kPrimaryEveryBatch};
  int chain = 0;
  for (int n = 1; n <= 6; ++n)
    for (int second_plane = 0; second_plane < 2; ++second_plane)
      for (int metric = 0; metric < 3; ++metric)  // 0: no batch carries the metric, 1: every batch, 2: the odd ones (it starts and stops in mid-call)
        for (int sw = 0; sw < 16; ++sw)
          for (int fused = 0; fused < 2; ++fused)
            for (int init = 0; init < 3; ++init)  // 0: nothing waits when the call begins, 1 / 2: a batch waits in plane 0 / 1
              for (int keys = 0; keys < 1 << n; ++keys, ++chain) {
                int flags = 0;
                for (int j = 0; j < 4; ++j) flags |= sw >> j & 1 ? switches[j] : 0;
                // a cornell-like batch: the ladder turns the switches into the form
                FormInputs fi{};
                fi.primary_share = 64, fi.trace_depth = 8, fi.debug_flags = flags, fi.num_mats = 5, fi.slot_shift = 21, fi.K = 25, fi.seg_cap = 8128;
                GatherInputs in{};
                in.form = batch_form(fi), in.second_plane = second_plane != 0, in.debug_flags = flags, in.fused = fused != 0;
                in.waiting = init != 0, in.waiting_plane = init == 2;
                for (int i = 0; i < n; ++i) {
                  in.after = n - 1 - i, in.same_key = (keys >> i & 1) != 0, in.metric = metric == 1 || (metric == 2 && (i & 1));
                  const GatherPlan p = gather_plan(in);
                  printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", chain, n, i, in.after, second_plane, (int)in.metric, flags, fused, (int)in.same_key,
                         (int)in.form.fixed_slots, (int)in.form.primary_once, (int)in.waiting, in.waiting_plane, p.form, (int)p.gathers_waiting, (int)p.defers, p.plane, p.reported,
                         (int)p.closing);
                  // run_batch: a waiting batch is gathered by this batch's k_paths or by a launch before it; this batch waits if it defers
                  in.waiting = p.defers, in.waiting_plane = p.defers ? p.plane : 0;
                }
              }
  return 0;
}
