// Host test of the planner's SCAFFOLD record (fl_round_plan.h), built with AddressSanitizer + UBSan: with the trait
// on the record sits between local step 0's TRAIN and ADAM, once per round whatever local_steps; off: absent.
#include <cstdio>

#include "fl_round_plan.h"

int main() {
    int failures = 0;
    for (int ls : {1, 5})
        for (int on = 0; on < 2; ++on) {
            RoundTraits t;
            t.world = 4;
            t.local_steps = ls;
            t.scaffold_on = on != 0;
            RoundCarry c;
            for (int r = 0; r < 3; ++r) {
                RoundPlan p;
                plan_round(t, c, p, r, false, false, false, false);   // FLEngine::run_local
                int n = 0, at = -1;
                for (int k = 0; k < p.n; ++k)
                    if (p.rec[k].kind == FLLaunchRec::SCAFFOLD) { ++n; at = k; }
                bool ok = n == on;
                if (on && ok)
                    ok = at >= 1 && at + 1 < p.n && p.rec[at - 1].kind == FLLaunchRec::TRAIN && p.rec[at - 1].i[0] == 0 &&
                         p.rec[at + 1].kind == FLLaunchRec::ADAM && p.rec[at + 1].i[0] == 0 &&
                         p.rec[at].p[0] == fl_at(FL_TB_ST0 + (r & 1));
                if (!ok) {
                    ++failures;
                    std::printf("FAIL local_steps %d on %d round %d: %d records, at %d of %d\n", ls, on, r, n, at, p.n);
                }
            }
        }
    std::printf("failures: %d\n", failures);
    return failures == 0 ? 0 : 1;
}
