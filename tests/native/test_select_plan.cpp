// Host test of the round plans of a selecting peer engine (gather_plane = "xgmi": a robust rule or
// secure aggregation inside the one-shot xGMI peer kernel), built with AddressSanitizer + UBSan.  Such an
// engine adds no launch kind and no planner case (fedmi/ops/csrc/fl_round_plan.h is unchanged): it is a
// peer engine whose traits are has_peer, !lag_ok, !xchg, !eval_fedavg_fits, and whose executor turns
// the ALLREDUCE record into the select / mask + open launches (fl_engine.cpp).  This pins the record
// sequence those traits give, fp32 and bf16, with and without a server optimizer, compression or DP
// (secure aggregation composes with DP), one and two local steps:
//
//   [PACK: bf16, first round only] (TRAIN ADAM) x local_steps [DP | COMPRESS] EVAL ALLREDUCE [SERVER]
//
// one ALLREDUCE per round on the round's output parity, no EVAL_FEDAVG, SERVER last when on; the
// contribution and the evaluation's tails go to the peer's send buffer of that parity.  The step API's
// phases give the same records, and such rounds are graph-capturable from round 0.
//
// usage: test_select_plan
#include <cstdio>
#include <vector>

#include "fl_round_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            ++failures;                        \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                 \
        }                                      \
    } while (0)

static RoundTraits select_traits(int dtype, int world, int local_steps, bool server, bool compress, bool dp) {
    RoundTraits t;
    t.dtype = dtype;
    t.world = world;
    t.local_steps = local_steps;
    t.has_peer = true;
    t.lag_ok = t.xchg = t.eval_fedavg_fits = t.fused = t.identity = false;
    t.server_on = server;
    t.compress_on = compress;
    t.dp_on = dp;
    return t;
}

static std::vector<int> expected(const RoundTraits& t, bool first_round) {
    std::vector<int> k;
    if (t.dtype == 1 && first_round) k.push_back(FLLaunchRec::PACK);
    for (int ls = 0; ls < t.local_steps; ++ls) {
        k.push_back(FLLaunchRec::TRAIN);
        k.push_back(FLLaunchRec::ADAM);
    }
    if (t.dp_on) k.push_back(FLLaunchRec::DP);
    else if (t.compress_on) k.push_back(FLLaunchRec::COMPRESS);
    k.push_back(FLLaunchRec::EVAL);
    k.push_back(FLLaunchRec::ALLREDUCE);
    if (t.server_on) k.push_back(FLLaunchRec::SERVER);
    return k;
}

static void check_round(const char* how, const RoundTraits& t, const RoundPlan& p, int r, bool first_round) {
    const std::vector<int> want = expected(t, first_round);
    const int par = (r + 1) & 1;
    char tag[160];
    std::snprintf(tag, sizeof(tag), "%s dtype %d world %d steps %d server %d compress %d dp %d round %d", how, t.dtype,
                  t.world, t.local_steps, (int)t.server_on, (int)t.compress_on, (int)t.dp_on, r);
    CHECK(p.n == (int)want.size(), "%s: %d records, expected %zu", tag, p.n, want.size());
    int n_all = 0;
    for (int k = 0; k < p.n; ++k) {
        const FLLaunchRec& m = p.rec[k];
        if (k < (int)want.size()) CHECK(m.kind == want[k], "%s: record %d is kind %d, expected %d", tag, k, m.kind, want[k]);
        CHECK(m.kind != FLLaunchRec::EVAL_FEDAVG, "%s: an EVAL_FEDAVG record", tag);
        CHECK(m.par == par, "%s: record %d on parity %d", tag, k, m.par);
        if (m.kind == FLLaunchRec::PACK) CHECK(k == 0 && first_round, "%s: a PACK record at %d", tag, k);
        if (m.kind == FLLaunchRec::ADAM) {
            CHECK(m.peer == 0, "%s: an exchanging Adam launch", tag);
            CHECK(m.p[2] == fl_at(FL_TB_COMM0 + par), "%s: the contribution does not go to the send buffer", tag);
        }
        if (m.kind == FLLaunchRec::DP || m.kind == FLLaunchRec::COMPRESS)
            CHECK(m.p[2] == fl_at(FL_TB_COMM0 + par) && m.p[3] == fl_at(FL_TB_ST0 + par), "%s: DP / COMPRESS buffers", tag);
        if (m.kind == FLLaunchRec::EVAL)
            CHECK(m.p[1] == fl_at(FL_TB_COMM0 + par) && m.p[2] == fl_at(FL_TB_ST0 + par), "%s: EVAL buffers", tag);
        if (m.kind == FLLaunchRec::ALLREDUCE) {
            ++n_all;
            CHECK(m.p[0] == fl_at(FL_TB_PBUF0 + par), "%s: ALLREDUCE output buffer", tag);
        }
        if (m.kind == FLLaunchRec::SERVER) {
            CHECK(k == p.n - 1, "%s: SERVER is not last", tag);
            CHECK(m.p[0] == fl_at(FL_TB_PBUF0 + (r & 1)) && m.p[1] == fl_at(FL_TB_PBUF0 + par) &&
                      m.p[2] == fl_at(FL_TB_ST0 + par),
                  "%s: SERVER buffers", tag);
        }
    }
    CHECK(n_all == 1, "%s: %d ALLREDUCE records", tag, n_all);
}

int main() {
    int checked = 0;
    for (int dtype = 0; dtype < 2; ++dtype)
        for (int world : {2, 3, 8})
            for (int steps = 1; steps <= 2; ++steps)
                for (int variant = 0; variant < 6; ++variant) {
                    // none | server | compress | compress + server | dp (secure aggregation) | dp + server
                    const bool server = variant & 1, compress = variant == 2 || variant == 3, dp = variant >= 4;
                    const RoundTraits t = select_traits(dtype, world, steps, server, compress, dp);
                    CHECK(!t.lagged() && !t.late_fold() && t.aggregates(false), "traits of a selecting engine");
                    // whole rounds, as run() and a graph capture issue them (no communicator object: the peer reduces)
                    RoundCarry c;
                    CHECK(!needs_eager_round(t, c), "a selecting engine captures from round 0");
                    for (int r = 0; r < 5; ++r) {
                        RoundPlan p;
                        plan_round(t, c, p, r, true, true, true, false);
                        check_round("run", t, p, r, r == 0);
                        CHECK(c.cm_in_tail && !c.pending_cm && !c.prev_lagged && !c.need_pack, "carry after round %d: %d", r,
                              c.bits());
                        CHECK(!needs_eager_round(t, c), "round %d leaves a capturable state", r);
                        ++checked;
                    }
                    // the same rounds through the step API's phases
                    RoundCarry s;
                    for (int r = 0; r < 3; ++r) {
                        RoundPlan p;
                        plan_phase(t, s, p, r, 0, false);
                        plan_phase(t, s, p, r, 1, false);
                        plan_phase(t, s, p, r, 2, false);
                        check_round("phases", t, p, r, r == 0);
                        ++checked;
                    }
                    // a host-side weight change repacks once (bf16)
                    s.need_pack = true;
                    RoundPlan p;
                    plan_round(t, s, p, 3, true, true, true, false);
                    check_round("after invalidate", t, p, 3, true);
                    // the closing finalize folds the tail region alone
                    RoundPlan f;
                    plan_finalize(t, s, f, 4);
                    CHECK(f.n == 1 && f.rec[0].kind == FLLaunchRec::FINALIZE && f.rec[0].i[0] == FL_FOLD_B, "finalize");
                }
    std::printf("select plan rounds checked: %d\n", checked);
    std::printf("select plan failures: %d\n", failures);
    return failures == 0 ? 0 : 1;
}
