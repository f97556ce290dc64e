// Host test of the round planner (fedmi/ops/csrc/fl_round_plan.h), built with AddressSanitizer + UBSan.
//
// 1. Golden sequences: tests/golden/round_plans.json holds, per engine configuration and call
//    script, the launches (kind, four ints) an engine issued on the GPU and its carry bits after
//    every call, recorded before the planner existed.  The scripts are replayed through the
//    planner with the engine's (thin) glue re-stated below; every launch and carry must be equal.
//    (Provenance: the recording build was that older engine plus a line written to a file after
//    every launch and `srv_packed_` added to flags() as bit 64, which flags() did not report
//    then; "traits" are the recording script's description of each configuration -- from the
//    EngineConfig it built and the engine's fused / lagged / adam_exchange / has_peer / layout()
//    -- in this header's field names, with comm_present = an RCCL communicator was passed.)
// 2. Invariants, after every call of every script: each issued round's metrics are produced at
//    most once and folded at most once, never folded before they are produced, and after
//    finalize every issued round was produced once and folded once.
// 3. finalize behind a lagged round throws; the steady carry needs no eager round; carry bits
//    round-trip; a full record array throws instead of writing past its end.
//
// usage: test_round_plan <round_plans.json>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "fl_round_plan.h"

// ---- a JSON reader for the golden file: objects, arrays, strings without escapes, integers, booleans ----
struct J {
    enum { NUM, STR, BOOL, ARR, OBJ } t = NUM;
    long long n = 0;
    std::string s;
    std::vector<J> a;
    std::map<std::string, J> o;
    const J& operator[](const char* k) const { return o.at(k); }
    const J& operator[](int i) const { return a.at((size_t)i); }
    const J& operator[](size_t i) const { return a.at(i); }
    bool b() const { return n != 0; }
};
struct Parser {
    const std::string& s;
    size_t i = 0;
    void ws() { while (i < s.size() && (s[i] == ' ' || s[i] == '\n' || s[i] == '\r' || s[i] == '\t')) ++i; }
    char peek() { ws(); if (i >= s.size()) throw std::runtime_error("json: truncated"); return s[i]; }
    void eat(char c) { if (peek() != c) throw std::runtime_error(std::string("json: expected ") + c); ++i; }
    J value() {
        J v;
        const char c = peek();
        if (c == '{') {
            v.t = J::OBJ;
            ++i;
            if (peek() == '}') { ++i; return v; }
            for (;;) {
                const std::string k = value().s;
                eat(':');
                v.o[k] = value();
                if (peek() == ',') { ++i; continue; }
                eat('}');
                return v;
            }
        }
        if (c == '[') {
            v.t = J::ARR;
            ++i;
            if (peek() == ']') { ++i; return v; }
            for (;;) {
                v.a.push_back(value());
                if (peek() == ',') { ++i; continue; }
                eat(']');
                return v;
            }
        }
        if (c == '"') {
            v.t = J::STR;
            const size_t e = s.find('"', ++i);
            if (e == std::string::npos) throw std::runtime_error("json: open string");
            v.s = s.substr(i, e - i);
            i = e + 1;
            return v;
        }
        if (s.compare(i, 4, "true") == 0) { v.t = J::BOOL; v.n = 1; i += 4; return v; }
        if (s.compare(i, 5, "false") == 0) { v.t = J::BOOL; i += 5; return v; }
        size_t used = 0;
        v.n = std::stoll(s.substr(i, 24), &used);
        i += used;
        return v;
    }
};

static int failures = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond);    \
            std::printf(__VA_ARGS__);                                      \
            std::printf("\n");                                             \
        }                                                                  \
    } while (0)

static const char* kKind[FLLaunchRec::N_KINDS] = {"PACK", "TRAIN", "ADAM", "EVAL", "ALLREDUCE", "EVAL_FEDAVG",
                                                  "DP", "SERVER", "FINALIZE"};

static RoundTraits traits_of(const J& t) {
    RoundTraits r;
    r.dtype = (int)t["dtype"].n;
    r.world = (int)t["world"].n;
    r.local_steps = (int)t["local_steps"].n;
    r.es_enabled = t["es_enabled"].b();
    r.fused = t["fused"].b();
    r.lag_ok = t["lag_ok"].b();
    r.xchg = t["xchg"].b();
    r.has_peer = t["has_peer"].b();
    r.emulate = t["emulate"].b();
    r.dp_on = t["dp_on"].b();
    r.server_on = t["server_on"].b();
    r.eval_fedavg_fits = t["eval_fedavg_fits"].b();
    r.identity = t["identity"].b();
    return r;
}

// The engine's glue around the planner (FLEngine::run / capture / replay), with the bookkeeping of
// which round every launch scores and folds.
struct Model {
    RoundTraits t;
    bool comm = false;
    RoundCarry c;
    std::vector<FLLaunchRec> all;        // every planned launch, in order
    std::map<int, int> produced, folded; // round -> times
    std::vector<FLLaunchRec> graph;      // launches of the captured rounds
    std::vector<int> graph_round;        // ... and the captured round index each belongs to
    int graph_n = 0, issued = 0;
    bool fold_before_score = false;

    void fold(int q) {
        if (q < 0) return;
        if (produced[q] == 0) fold_before_score = true;
        ++folded[q];
    }
    // launches of one planning call for round r (finalize: r = rounds issued, all folds, flush only)
    void account(const FLLaunchRec* b, const FLLaunchRec* e, int r, bool trained = false) {
        for (const FLLaunchRec* m = b; m != e; ++m) {
            if (m->kind == FLLaunchRec::EVAL || m->kind == FLLaunchRec::EVAL_FEDAVG) ++produced[trained ? r : r - 1];
            if (m->kind == FLLaunchRec::TRAIN) {
                trained = true;
                if (m->i[0] == 0 && (m->i[2] == FL_EVAL_FUSED || m->i[2] == FL_EVAL_LAGGED)) ++produced[r - 1];
            }
            const bool folds = m->kind == FLLaunchRec::FINALIZE || (m->kind == FLLaunchRec::ADAM && m->i[1] == 1);
            const int mask = m->kind == FLLaunchRec::FINALIZE ? m->i[0] : m->i[3];
            if (folds && (mask & FL_FOLD_A)) fold(r - 2);
            if (folds && (mask & FL_FOLD_B)) fold(r - 1);
            if (m->kind == FLLaunchRec::ADAM && (m->peer & 4)) fold(r - 1);
        }
    }
    void keep(const RoundPlan& p) { all.insert(all.end(), p.begin(), p.end()); }
    void round(int r, bool allow_fused, bool lag, bool server, bool comm_present, bool capturing = false) {
        RoundPlan p;
        plan_round(t, c, p, r, allow_fused, lag, server, comm_present);
        keep(p);
        if (!capturing) {
            account(p.begin(), p.end(), r);
            issued = r + 1;
        } else {
            graph.insert(graph.end(), p.begin(), p.end());
            graph_round.insert(graph_round.end(), (size_t)p.n, r);
        }
    }
    void op(const J& o) {
        const std::string& what = o[0].s;
        if (what == "run") {
            const int r0 = (int)o[1].n, n = (int)o[2].n;
            for (int r = r0; r < r0 + n; ++r) round(r, true, t.lagged() && !(o[3].n != 0 && r == r0 + n - 1), true, comm);
        } else if (what == "run_local") {
            round((int)o[1].n, false, false, false, false);
        } else if (what == "phase") {
            RoundPlan p;
            const int r = (int)o[1].n, which = (int)o[2].n;
            plan_phase(t, c, p, r, which, comm);
            keep(p);
            // phase 1 scores round r itself: its EVAL counts as "after the train launch"
            account(p.begin(), p.end(), r, which == 1);
            if (which == 2 || which == 3) issued = r + 1;
        } else if (what == "finalize") {
            RoundPlan p;
            plan_finalize(t, c, p, (int)o[1].n);
            keep(p);
            account(p.begin(), p.end(), (int)o[1].n);
            for (int q = 0; q < issued; ++q)
                CHECK(produced[q] == 1 && folded[q] == 1, "round %d produced %d folded %d after finalize", q,
                      produced[q], folded[q]);
        } else if (what == "invalidate") {
            c.need_pack = true;
        } else if (what == "capture") {
            CHECK(!needs_eager_round(t, c), "capture from a carry that needs an eager round");
            const RoundCarry c0 = c;
            graph.clear();
            graph_round.clear();
            graph_n = (int)o[1].n;
            for (int r = 0; r < graph_n; ++r) round(r, true, t.lagged(), true, comm, true);
            c = c.with_metrics_of(c0);
        } else if (what == "replay") {
            CHECK(!needs_eager_round(t, c), "replay from a carry that needs an eager round");
            const int base = issued;
            for (size_t k = 0; k < graph.size();) {
                size_t e = k;
                while (e < graph.size() && graph_round[e] == graph_round[k]) ++e;
                account(&graph[k], &graph[k] + (e - k), base + graph_round[k]);
                k = e;
            }
            issued = base + graph_n;
            c = c.steady(t);
        } else {
            throw std::runtime_error("unknown script op " + what);
        }
        for (auto& [q, n] : produced) CHECK(n <= 1, "round %d produced %d times", q, n);
        for (auto& [q, n] : folded) CHECK(n <= 1, "round %d folded %d times", q, n);
        CHECK(!fold_before_score, "a round was folded before it was scored");
    }
};

static void check_golden(const J& rec) {
    const std::string name = rec["config"].s + "/" + rec["script_name"].s;
    Model m;
    m.t = traits_of(rec["traits"]);
    m.comm = rec["traits"]["comm_present"].b();
    const J& script = rec["script"];
    const J& carries = rec["carry_after_each_op"];
    for (size_t k = 0; k < script.a.size(); ++k) {
        m.op(script[k]);
        CHECK(m.c.bits() == (int)carries[k].n, "%s: carry %d after call %zu, recorded %lld", name.c_str(), m.c.bits(), k,
              carries[k].n);
    }
    CHECK(m.c.bits() == (int)rec["final_carry"].n, "%s: final carry", name.c_str());
    const J& want = rec["launches"];
    CHECK(m.all.size() == want.a.size(), "%s: %zu launches planned, %zu recorded", name.c_str(), m.all.size(),
          want.a.size());
    for (size_t k = 0; k < m.all.size() && k < want.a.size(); ++k) {
        const FLLaunchRec& g = m.all[k];
        const J& w = want[k];
        CHECK(w[0].s == kKind[g.kind] && w[1].n == g.i[0] && w[2].n == g.i[1] && w[3].n == g.i[2] && w[4].n == g.i[3],
              "%s: launch %zu planned %s %d %d %d %d, recorded %s %lld %lld %lld %lld", name.c_str(), k, kKind[g.kind],
              g.i[0], g.i[1], g.i[2], g.i[3], w[0].s.c_str(), w[1].n, w[2].n, w[3].n, w[4].n);
    }
    // independent of the script: this configuration's steady state, and finalize behind a lagged round
    CHECK(!needs_eager_round(m.t, RoundCarry{}.steady(m.t)), "%s: steady carry needs an eager round", name.c_str());
    if (m.t.lagged()) {
        RoundCarry c;
        RoundPlan p;
        plan_round(m.t, c, p, 0, true, true, true, m.comm);
        bool threw = false;
        try {
            plan_finalize(m.t, c, p, 1);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        CHECK(threw, "%s: finalize behind a lagged round did not throw", name.c_str());
    }
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: test_round_plan <round_plans.json>\n");
        return 2;
    }
    std::ifstream f(argv[1]);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    Parser ps{text};
    const J golden = ps.value();
    for (const J& rec : golden.a) check_golden(rec);

    for (int b = 0; b < 128; ++b) CHECK(RoundCarry::from_bits(b).bits() == b, "carry bits %d", b);
    CHECK(RoundCarry{}.bits() == 32, "a new engine only has a repack pending");
    {
        const RoundCarry c = RoundCarry::from_bits(127).cleared();
        CHECK(c.bits() == (32 | 64), "cleared() keeps the pack state only: %d", c.bits());
    }
    {
        // exact-size heap object: ASan sees any write past the record array
        std::unique_ptr<RoundPlan> p(new RoundPlan);
        for (int k = 0; k < FL_PLAN_CAP; ++k) p->push(FLLaunchRec::EVAL, 0, 0, 0, 0, 0, fl_at(FL_TB_LOCAL));
        bool threw = false;
        try {
            p->push(FLLaunchRec::EVAL, 0, 0, 0, 0, 0, fl_at(FL_TB_LOCAL));
        } catch (const std::runtime_error&) {
            threw = true;
        }
        CHECK(threw && p->n == FL_PLAN_CAP, "overflowing push");
        std::unique_ptr<RoundPlan> q(new RoundPlan);
        RoundTraits t;
        t.dtype = 1;
        t.local_steps = FL_PLAN_MAX_LOCAL_STEPS;
        t.dp_on = t.server_on = t.emulate = true;
        RoundCarry c;
        plan_round(t, c, *q, 0, true, false, true, true);
        CHECK(q->n == 2 * t.local_steps + 5 && q->n <= FL_PLAN_CAP, "largest planned round: %d records", q->n);
        t.local_steps = FL_PLAN_CAP;
        q->n = 0;
        threw = false;
        try {
            plan_round(t, c, *q, 1, true, false, true, true);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        CHECK(threw, "a round with too many local steps");
    }
    std::printf("max local steps: %d\n", FL_PLAN_MAX_LOCAL_STEPS);
    std::printf("sequences checked: %zu\nfailures: %d\n", golden.a.size(), failures);
    return failures == 0 ? 0 : 1;
}
