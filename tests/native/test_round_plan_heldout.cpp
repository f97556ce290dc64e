// Host test of the round planner's held-out record (fedmi/ops/csrc/fl_round_plan.h: RoundTraits::heldout_on,
// FLLaunchRec::HELDOUT, plan_phase 4), built with AddressSanitizer + UBSan beside test_round_plan.cpp.
//
// Over a grid of engine traits -- dtype, world, local steps, server optimizer, DP, compression, peer
// plane, in-kernel exchange, lagged layout, early stopping, fused evaluation, emulation, RCCL present --
// and several rounds of each:
// 1. Trait on: every round the engine aggregates itself ends with exactly one HELDOUT record, on the
//    output parity's image and state; rounds the caller aggregates (run_local, or no data plane) hold
//    none, and phase 4 plans exactly that one record (phase 2 ends with it when the engine aggregates).
// 2. Trait on: no configuration is lagged or folds late, no train launch runs in lagged mode, and
//    asking for a lagged round plans a classic one -- so no round a late fold could discard leaves a row.
// 3. Trait off: no HELDOUT record anywhere, and wherever the trait does not change the round kind
//    (no lagged rounds) the trait-on plan without its HELDOUT records is the trait-off plan, record for
//    record and carry for carry.  (That trait-off plans equal the sequences recorded before the field
//    existed is test_round_plan.cpp's golden check, which runs unchanged.)
//
// usage: test_round_plan_heldout
#include <cstdio>
#include <vector>

#include "fl_round_plan.h"

static int failures = 0;
static long long checked = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        ++checked;                                                         \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond);    \
            std::printf(__VA_ARGS__);                                      \
            std::printf("\n");                                             \
        }                                                                  \
    } while (0)

static int count_kind(const RoundPlan& p, int kind) {
    int n = 0;
    for (const FLLaunchRec& m : p) n += m.kind == kind;
    return n;
}
static bool same_rec(const FLLaunchRec& a, const FLLaunchRec& b) { return same_launch(a, b) && same_buffers(a, b); }

static void check_traits(RoundTraits t, bool comm, int id) {
    const int ROUNDS = 6;
    RoundTraits off = t, on = t;
    off.heldout_on = false;
    on.heldout_on = true;
    // 2. never lagged, never a late fold
    CHECK(!on.lagged() && !on.late_fold(), "config %d: lagged %d late_fold %d with held-out scoring", id, on.lagged(),
          on.late_fold());
    RoundCarry c_on, c_off;
    for (int r = 0; r < ROUNDS; ++r) {
        const bool last = r == ROUNDS - 1;
        RoundPlan p_on, p_off;
        // as FLEngine::run issues rounds; the trait-on engine is ASKED for lagged rounds too
        plan_round(on, c_on, p_on, r, true, !last, true, comm);
        plan_round(off, c_off, p_off, r, true, off.lagged() && !last, true, comm);
        const int par = (r + 1) & 1;
        const int n_ho = count_kind(p_on, FLLaunchRec::HELDOUT);
        if (on.aggregates(comm)) {
            // 1. exactly one, last, on the output parity
            CHECK(n_ho == 1, "config %d round %d: %d HELDOUT records", id, r, n_ho);
            const FLLaunchRec& m = p_on.rec[p_on.n - 1];
            CHECK(m.kind == FLLaunchRec::HELDOUT, "config %d round %d: the round ends with kind %d", id, r, m.kind);
            CHECK(m.par == par && m.p[0] == fl_at(FL_TB_PBUF0 + par) && m.p[1] == fl_at(FL_TB_ST0 + par),
                  "config %d round %d: HELDOUT reads base %d / %d, parity %d", id, r, m.p[0].base, m.p[1].base, m.par);
            if (on.server_on)
                CHECK(p_on.n >= 2 && p_on.rec[p_on.n - 2].kind == FLLaunchRec::SERVER,
                      "config %d round %d: HELDOUT does not follow the server step", id, r);
        } else {
            CHECK(n_ho == 0, "config %d round %d: %d HELDOUT records in a round the caller aggregates", id, r, n_ho);
        }
        for (const FLLaunchRec& m : p_on)
            CHECK(!(m.kind == FLLaunchRec::TRAIN && m.i[2] == FL_EVAL_LAGGED) && !(m.kind == FLLaunchRec::ADAM && m.peer),
                  "config %d round %d: a lagged launch with held-out scoring", id, r);
        CHECK(!c_on.prev_lagged, "config %d round %d: the round was planned lagged", id, r);
        // 3. trait off
        CHECK(count_kind(p_off, FLLaunchRec::HELDOUT) == 0, "config %d round %d: HELDOUT with the trait off", id, r);
        if (!off.lagged()) {
            int k = 0;
            bool same = true;
            for (const FLLaunchRec& m : p_on) {
                if (m.kind == FLLaunchRec::HELDOUT) continue;
                same = same && k < p_off.n && same_rec(m, p_off.rec[k]);
                ++k;
            }
            CHECK(same && k == p_off.n, "config %d round %d: plans differ beyond the HELDOUT record", id, r);
            CHECK(c_on.bits() == c_off.bits(), "config %d round %d: carry %d vs %d", id, r, c_on.bits(), c_off.bits());
        }
        // rounds the caller aggregates (FLEngine::run_local): none
        RoundCarry c2 = c_on;
        RoundPlan p_loc;
        plan_round(on, c2, p_loc, r + 1, false, false, false, false);
        CHECK(count_kind(p_loc, FLLaunchRec::HELDOUT) == 0, "config %d: HELDOUT in run_local", id);
    }
    // finalize works behind the last (self-evaluating) round
    {
        RoundPlan p;
        plan_finalize(on, c_on, p, ROUNDS);
        CHECK(count_kind(p, FLLaunchRec::HELDOUT) == 0 && count_kind(p, FLLaunchRec::FINALIZE) == 1, "config %d: finalize",
              id);
    }
    // phases
    {
        RoundCarry c;
        RoundPlan p0, p1, p2, p4;
        plan_phase(on, c, p0, 0, 0, comm);
        plan_phase(on, c, p1, 0, 1, comm);
        plan_phase(on, c, p2, 0, 2, comm);
        CHECK(count_kind(p0, FLLaunchRec::HELDOUT) == 0 && count_kind(p1, FLLaunchRec::HELDOUT) == 0,
              "config %d: HELDOUT in phase 0 / 1", id);
        CHECK(count_kind(p2, FLLaunchRec::HELDOUT) == (on.aggregates(comm) ? 1 : 0) &&
                  (!on.aggregates(comm) || p2.rec[p2.n - 1].kind == FLLaunchRec::HELDOUT),
              "config %d: phase 2", id);
        plan_phase(on, c, p4, 0, 4, comm);
        CHECK(p4.n == 1 && p4.rec[0].kind == FLLaunchRec::HELDOUT && p4.rec[0].par == 1 &&
                  p4.rec[0].p[0] == fl_at(FL_TB_PBUF1) && p4.rec[0].p[1] == fl_at(FL_TB_ST1),
              "config %d: phase 4", id);
        bool threw = false;
        RoundPlan q;
        try {
            plan_phase(off, c, q, 0, 4, comm);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        CHECK(threw && q.n == 0, "config %d: phase 4 without a held-out set", id);
        RoundPlan q2;
        plan_phase(off, c, q2, 0, 2, comm);
        CHECK(count_kind(q2, FLLaunchRec::HELDOUT) == 0, "config %d: phase 2 with the trait off", id);
    }
}

int main() {
    int id = 0, lag_cfgs = 0, late_cfgs = 0;
    for (int dtype = 0; dtype < 2; ++dtype)
    for (int world : {1, 2, 4})
    for (int ls : {1, 3})
    for (int foreign = 0; foreign < 4; ++foreign)   // 0 none, 1 DP, 2 compression, 3 neither + server below
    for (int server = 0; server < 2; ++server)
    for (int peer = 0; peer < 2; ++peer)
    for (int lag_ok = 0; lag_ok < 2; ++lag_ok)
    for (int es = 0; es < 2; ++es)
    for (int comm = 0; comm < 2; ++comm)
    for (int emulate = 0; emulate < 2; ++emulate) {
        if (foreign == 3) continue;
        RoundTraits t;
        t.dtype = dtype;
        t.world = world;
        t.local_steps = ls;
        t.cm_off = 4 * 1000;
        t.es_enabled = es;
        t.dp_on = foreign == 1;
        t.compress_on = foreign == 2;
        t.server_on = server;
        t.has_peer = peer;
        t.emulate = emulate;
        t.identity = world == 1 && !emulate;
        // the engine's own rules (fl_engine.cpp): fused needs one client and a plain output; lagged
        // layouts are bf16, several (or emulated) clients, a plain output, never fused
        t.fused = t.identity && !t.foreign_output() && !peer && lag_ok == 0;
        t.lag_ok = lag_ok && dtype == 1 && (world > 1 || emulate) && !t.foreign_output() && !t.fused;
        t.xchg = t.lag_ok && peer && ls == 1;
        t.eval_fedavg_fits = peer && (id & 1);
        if (peer && comm) continue;   // an engine with a peer plane never takes an RCCL communicator
        lag_cfgs += t.lagged();
        late_cfgs += t.late_fold();
        check_traits(t, comm != 0, id++);
    }
    // the grid must hold what the rules are about: lagged and late-fold configurations with the trait off
    CHECK(lag_cfgs > 0 && late_cfgs > 0, "grid: %d lagged, %d late-fold configurations", lag_cfgs, late_cfgs);
    // a largest round with the record still fits the plan
    {
        RoundPlan q;
        RoundTraits t;
        t.dtype = 1;
        t.local_steps = FL_PLAN_MAX_LOCAL_STEPS;
        t.dp_on = t.server_on = t.emulate = t.heldout_on = true;
        RoundCarry c;
        plan_round(t, c, q, 0, true, false, true, true);
        CHECK(q.n == 2 * t.local_steps + 6 && q.n <= FL_PLAN_CAP, "largest planned round: %d records", q.n);
    }
    std::printf("configurations: %d\nchecks: %lld\nfailures: %d\n", id, checked, failures);
    return failures == 0 ? 0 : 1;
}
