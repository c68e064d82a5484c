// Prints the form ladder of csrc/pt_sched.h — batch_form over the cross-product of its conditions, directly and through a BatchInfo
// (form_inputs), with the gather form each result leads to — for tests/test_sched_form.py, which compiles this with the system
// compiler, runs it and checks the output against its own restatement of the ladder.  Output: header lines `name key=value ...`;
// behind `table` one line of plain numbers per case.
#include <cstdint>
#include <cstdio>

#include "pt_lds.h"
#include "pt_sched.h"

using namespace ptk;

static int packed(const BatchForm& f) {
  return (int)f.shares | (int)f.retire_once << 1 | f.records << 2 | (int)f.fixed_slots << 4 | (int)f.primary_once << 5 | f.split << 6;
}
static int gather_of(const BatchForm& f, int flags, bool metric) {
  GatherInputs in{};
  in.form = f, in.metric = metric, in.debug_flags = flags, in.fused = true;
  return gather_plan(in).form;
}

int main() {
  printf("consts trace_every_iteration=%d every_iteration=%d whole=%d no_first=%d by_visit=%d tile=%d every_batch=%d gather_every_batch=%d split=%d first=%d template=%d "
         "forms=%d,%d,%d,%d lds_tables=%d search_lds_tables=%d visit_bits=%d no_second_plane=%d\n",
         kTraceEveryIteration, kRetireEveryIteration, kWholeRecords, kNoFirstBounce, kRecordsByVisit, kTileGather, kPrimaryEveryBatch, kGatherEveryBatch, kSplitRecords,
         kFirstBounce, kFixedSlots, kGatherTile, kGatherTileFixed, kGatherStream, kGatherInline, (int)kLdsTables, kSearchLdsTables, kVisitBits, kNoSecondPlane);
  // table: every value any of the earlier per-rung sweeps gave a condition, crossed.  slot_shift 28: 2^(31 - 28) = 8 material indices
  // fit; seg_cap 8128: 13 bits, 2^18 iterations fit beside the slot; 2^(31 - kVisitBits) fit beside the visit number.
  const int shift = 28, seg_cap = 8128, vmax = 1 << (31 - kVisitBits);
  printf("table shift=%d seg_cap=%d cols=share,aa,flat,depth,flags,form,mats,K,direct,through_b,gather,gather_metric\n", shift, seg_cap);
  for (int share : {-1, 0, 1, 2, 25, 64})
    for (int aa = 0; aa < 2; ++aa)
      for (int flat = 0; flat < 2; ++flat)
        for (int depth : {1, 2, 3, 8})
          for (int flags : {0, 16, 128, 1024, 1024 | 16, 2048 | 512, 4096, 4096 | 16, 8192, 8192 | 4096, 8192 | 1024, 16384, 32768, 16384 | 32768, 16384 | 16,
                            32768 | 8192, 65536, 65536 | 16, 65536 | 32768, 65536 | 16384})
            for (int form : {0, 1, 2})
              for (int mats : {1, 8, 9})
                for (int K : {1, 3, 25, 1 << 18, (1 << 18) + 1, vmax, vmax + 1}) {
                  FormInputs in{};
                  in.primary_share = share, in.aa_jitter = aa != 0, in.flat = flat != 0, in.trace_depth = depth, in.debug_flags = flags, in.search_form = form;
                  in.num_mats = mats, in.slot_shift = shift, in.K = K, in.seg_cap = seg_cap;
                  BatchInfo b{};
                  b.primary_share = share, b.aa_jitter = aa, b.flat = flat, b.trace_depth = depth, b.slot_shift = shift, b.K = K;
                  const BatchForm f = batch_form(in), fb = batch_form(form_inputs(b, flags, form, mats, seg_cap));
                  printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", share, aa, flat, depth, flags, form, mats, K, packed(f) | (int)primary_shares(b) << 8, packed(fb),
                         gather_of(f, flags, false), gather_of(f, flags, true));
                }
  // a shorter batch of the same plan: the rule that holds for the plan's K holds for every batch length below it
  for (int cap : {64, 8128, 1 << 20})
    for (int K : {1, 2, 25, 256, 1 << 10, 1 << 12})
      for (int kb : {1, K / 2 > 0 ? K / 2 : 1, K}) {
        FormInputs in{};
        in.primary_share = 64, in.trace_depth = 8, in.num_mats = 5, in.slot_shift = 21, in.seg_cap = cap;
        in.K = K;
        const bool once_K = batch_form(in).primary_once;
        in.K = kb;
        printf("shorter seg_cap=%d K=%d kb=%d once_K=%d once_kb=%d\n", cap, K, kb, (int)once_K, (int)batch_form(in).primary_once);
      }
  BatchInfo zero{};
  printf("fresh retire_once=%d split_records=%d fixed_slots=%d size=%d\n", (int)zero.retire_once, (int)zero.split_records, (int)zero.fixed_slots, (int)sizeof(BatchInfo));
  return 0;
}
