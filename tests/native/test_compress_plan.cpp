// Host test of the COMPRESS launch kind of the round planner (fedmi/ops/csrc/fl_round_plan.h), built
// with AddressSanitizer + UBSan.  Re-uses the golden reader, the engine glue model and the golden check
// of test_round_plan.cpp (included with its main renamed; that file stays as it is).
//
// 1. With compress_on false (every golden configuration) the plans are record for record the recorded
//    ones: the whole golden check runs again against this header, and no plan holds a COMPRESS record.
// 2. With compress_on in place of dp_on (the golden DP configurations, every script: run / close,
//    step API, invalidate, capture + replay) the plan is the DP plan with every DP record replaced by a
//    COMPRESS record -- same position, same scalars, same buffers -- and the same carry after every call.
// 3. Several clients, two local steps, a server optimizer, the step API: one COMPRESS record per round,
//    directly behind the round's last ADAM record, reading (local, round input, comm buffer, state).
// 4. compress_on makes the output foreign; the largest planned round still fits the record array.
//
// usage: test_compress_plan <round_plans.json>
#define main round_plan_golden_main
#include "test_round_plan.cpp"
#undef main

static int count_kind(const std::vector<FLLaunchRec>& v, int kind) {
    int n = 0;
    for (const FLLaunchRec& m : v) n += m.kind == kind;
    return n;
}

static void check_swapped(const J& rec) {
    const std::string name = rec["config"].s + "/" + rec["script_name"].s;
    Model a, b;
    a.t = b.t = traits_of(rec["traits"]);
    a.comm = b.comm = rec["traits"]["comm_present"].b();
    b.t.dp_on = false;
    b.t.compress_on = true;
    const J& script = rec["script"];
    for (size_t k = 0; k < script.a.size(); ++k) {
        a.op(script[k]);
        b.op(script[k]);
        CHECK(a.c.bits() == b.c.bits(), "%s: carry %d with DP, %d with compression after call %zu", name.c_str(),
              a.c.bits(), b.c.bits(), k);
    }
    CHECK(a.all.size() == b.all.size(), "%s: %zu launches with DP, %zu with compression", name.c_str(), a.all.size(),
          b.all.size());
    CHECK(count_kind(a.all, FLLaunchRec::DP) > 0 && count_kind(b.all, FLLaunchRec::DP) == 0 &&
              count_kind(b.all, FLLaunchRec::COMPRESS) == count_kind(a.all, FLLaunchRec::DP),
          "%s: %d DP records, %d COMPRESS records", name.c_str(), count_kind(a.all, FLLaunchRec::DP),
          count_kind(b.all, FLLaunchRec::COMPRESS));
    for (size_t k = 0; k < a.all.size() && k < b.all.size(); ++k) {
        FLLaunchRec want = a.all[k];
        if (want.kind == FLLaunchRec::DP) want.kind = FLLaunchRec::COMPRESS;
        CHECK(same_launch(want, b.all[k]) && same_buffers(want, b.all[k]), "%s: launch %zu differs (kind %d / %d)",
              name.c_str(), k, want.kind, b.all[k].kind);
    }
}

int main(int argc, char** argv) {
    const int rc = round_plan_golden_main(argc, argv);  // compress_on false: the recorded plans
    if (rc == 2) return rc;
    std::ifstream f(argv[1]);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    Parser ps{text};
    const J golden = ps.value();
    int swapped = 0;
    for (const J& rec : golden.a) {
        Model m;
        m.t = traits_of(rec["traits"]);
        m.comm = rec["traits"]["comm_present"].b();
        for (size_t k = 0; k < rec["script"].a.size(); ++k) m.op(rec["script"][k]);
        CHECK(count_kind(m.all, FLLaunchRec::COMPRESS) == 0, "%s: a COMPRESS record without compress_on",
              rec["config"].s.c_str());
        if (m.t.dp_on) {
            check_swapped(rec);
            ++swapped;
        }
    }
    CHECK(swapped >= 5, "golden DP configurations replayed with compression: %d", swapped);
    {
        RoundTraits t;
        CHECK(!t.compress_on && !t.foreign_output(), "compression is off by default");
        t.compress_on = true;
        CHECK(t.foreign_output(), "a compressing engine's output is foreign");
    }
    for (int dtype = 0; dtype < 2; ++dtype) {
        // 4 clients aggregated by the caller, 2 local steps, server optimizer: rounds through the step API
        RoundTraits t;
        t.dtype = dtype;
        t.world = 4;
        t.local_steps = 2;
        t.compress_on = t.server_on = true;
        RoundCarry c;
        for (int r = 0; r < 5; ++r) {
            RoundPlan p;
            plan_phase(t, c, p, r, 0, false);
            const int in = r & 1, par = (r + 1) & 1;
            int n = 0, at = -1, last_adam = -1;
            for (int k = 0; k < p.n; ++k) {
                if (p.rec[k].kind == FLLaunchRec::COMPRESS) { ++n; at = k; }
                if (p.rec[k].kind == FLLaunchRec::ADAM) last_adam = k;
            }
            CHECK(n == 1 && at == p.n - 1 && at == last_adam + 1, "round %d: %d COMPRESS records, at %d of %d", r, n, at,
                  p.n);
            const FLLaunchRec& m = p.rec[at < 0 ? 0 : at];
            CHECK(m.par == par && m.p[0] == fl_at(FL_TB_LOCAL) && m.p[1] == fl_at(FL_TB_PBUF0 + in) &&
                      m.p[2] == fl_at(FL_TB_PBUF0 + par) && m.p[3] == fl_at(FL_TB_ST0 + par) && m.p[4].base == -1,
                  "round %d: COMPRESS buffers", r);
            // bf16: the server launch packs its own output, so only the first round stages a pack
            if (dtype == 1) CHECK((p.rec[0].kind == FLLaunchRec::PACK) == (r == 0), "round %d: bf16 pack", r);
            RoundPlan q;
            plan_phase(t, c, q, r, 1, false);
            plan_phase(t, c, q, r, 3, false);
            CHECK(count_kind(std::vector<FLLaunchRec>(q.begin(), q.end()), FLLaunchRec::COMPRESS) == 0,
                  "round %d: COMPRESS outside the training phase", r);
        }
    }
    {
        std::unique_ptr<RoundPlan> q(new RoundPlan);
        RoundTraits t;
        t.dtype = 1;
        t.local_steps = FL_PLAN_MAX_LOCAL_STEPS;
        t.compress_on = t.server_on = t.emulate = true;
        RoundCarry c;
        plan_round(t, c, *q, 0, true, false, true, true);
        CHECK(q->n == 2 * t.local_steps + 5 && q->n <= FL_PLAN_CAP, "largest planned round: %d records", q->n);
        // one client, bf16: a pack every round (the Adam-packed local image is not the input)
        RoundTraits o;
        o.dtype = 1;
        o.identity = true;
        o.compress_on = true;
        RoundCarry oc;
        for (int r = 0; r < 4; ++r) {
            RoundPlan p;
            plan_round(o, oc, p, r, true, false, true, false);
            CHECK(p.n == 5 && p.rec[0].kind == FLLaunchRec::PACK && p.rec[1].kind == FLLaunchRec::TRAIN &&
                      p.rec[1].i[1] == 0 && p.rec[2].kind == FLLaunchRec::ADAM && p.rec[3].kind == FLLaunchRec::COMPRESS &&
                      p.rec[4].kind == FLLaunchRec::EVAL,
                  "one bf16 client, round %d: %d records", r, p.n);
        }
    }
    std::printf("compress plan failures: %d\n", failures);
    return failures == 0 ? 0 : 1;
}
