// Prints csrc/pt_sched.h's queue_plan(m, Q, K) for EVERY m <= capacity of a few (capacity, Q, K) (tests/test_sched_capacity.py
// compiles this with the system compiler, runs it and checks the output by enumeration): a worker context planned for `capacity`
// pixels runs a list of m pixels under the plan of m in the buffers of the capacity's plan.  Output: one header line per case
// (`case capacity=.. Q=.. K=..`), then one line `m nq seg_cap cap` for m = 1 and for every m whose plan differs from that of m - 1.
#include <cstdint>
#include <cstdio>

#include "pt_sched.h"

using namespace ptk;

struct Case {
  int capacity, Q, K;
};
// 97 x 11 with 3 iterations per batch and 96 x 54 (whole and a quarter) with the automatic 256, all with the 256 queues of a
// 256-CU device; a quarter of 1920 x 1080 with its automatic 98; and smaller Q and K, a single queue among them
static const Case kCases[] = {{1067, 256, 3}, {1067, 256, 25}, {5184, 256, 256}, {1296, 256, 256}, {5184, 256, 4},
                              {518400, 256, 98}, {518400, 256, 25}, {518400, 1024, 98}, {5917, 4, 3}, {700, 1, 1}, {65, 1, 65}};

int main() {
  for (const Case& c : kCases) {
    printf("case capacity=%d Q=%d K=%d\n", c.capacity, c.Q, c.K);
    QueuePlan last{-1, -1, -1};
    for (int m = 1; m <= c.capacity; ++m) {
      const QueuePlan p = queue_plan(m, c.Q, c.K);
      if (p.nq != last.nq || p.seg_cap != last.seg_cap || p.cap != last.cap) printf("%d %d %d %d\n", m, p.nq, p.seg_cap, p.cap);
      last = p;
    }
  }
  return 0;
}
