// Host-only planner of the federated round engine: which kernels a round launches, with which
// mode, fold mask and buffers, as a pure function of the engine's fixed traits and a small carry
// (which metrics the last issued round left pending).  No HIP, no pybind: FLEngine executes the
// records (fl_engine.cpp), TrialBatch batches them over trials, and the same code runs in a host
// test binary with AddressSanitizer + UBSan (tests/native/test_round_plan.cpp).
#pragma once
#include <stdexcept>

// Evaluation placement of a round (`mode` of the train kernels).
//   FL_EVAL_CLASSIC : the train kernel folds the previous round's metrics into the state at
//                     its start; a separate eval kernel scores the post-step model.
//   FL_EVAL_FUSED   : one client (FedAvg is the identity, so the round's input weights ARE
//                     the previous round's post-step local model): the train kernel's own
//                     forward pass yields the previous round's confusion counts (argmax in
//                     the loss epilogue) and the Adam kernel folds them and decides whether
//                     this round is live.  No eval kernel.
//   FL_EVAL_FUSED_SKIP : as FUSED, but the previous round's counts are already in the tail
//                     (that round ran classic); the train kernel only trains.
#define FL_EVAL_CLASSIC 0
#define FL_EVAL_FUSED 1
#define FL_EVAL_FUSED_SKIP 2
//   FL_EVAL_LAGGED  : several clients: the train kernel of round r first scores round r-1's
//                     post-step LOCAL model (a forward pass on the staged local image, before
//                     the round's own weights replace it in LDS) into the local count buffer;
//                     the Adam kernel publishes those counts (+ round r-1's loss) in region A
//                     of round r's exchange, so no round needs a separate evaluation kernel.
//                     With the Adam-fused exchange region A is exchanged and folded inside
//                     round r's Adam kernel (in time for early stopping); riding an external
//                     all-reduce (RCCL) it is folded one round later, by round r+1's Adam
//                     kernel -- with early stopping round r runs before round r-1's stop is
//                     known and is then discarded bit-exactly (FLState::late).
#define FL_EVAL_LAGGED 3
// Metric regions of an all-reduced comm buffer that a fold consumes (fl_device.h).
#define FL_FOLD_A 1  // lag region: round next_round - 2
#define FL_FOLD_B 2  // tail region: round next_round - 1

// A buffer argument of a launch as (base slot, byte offset).  The first FL_TB_BASES slots are
// the pointer bases of a trial's device table (fl_common.h FLTrialDesc); FL_TB_COMM0 / 1 name
// the peer all-reduce's send buffer of that parity and exist only on the host (engines with a
// peer never join a trial batch).
#define FL_TB_BASES 8
enum { FL_TB_PBUF0 = 0, FL_TB_PBUF1, FL_TB_ST0, FL_TB_ST1, FL_TB_LOCAL, FL_TB_LAG, FL_TB_PKG, FL_TB_PKL,
       FL_TB_COMM0, FL_TB_COMM1 };
struct FLSel {
    int base;        // FL_TB_* slot, -1 = nullptr
    int pad;
    long long off;   // bytes
};
inline bool operator==(const FLSel& a, const FLSel& b) { return a.base == b.base && a.off == b.off; }

// One launch of a round.  The kinds double as trace tags (FLEngine::trace).
struct FLLaunchRec {
    enum Kind { PACK, TRAIN, ADAM, EVAL, ALLREDUCE, EVAL_FEDAVG, DP, SERVER, FINALIZE, COMPRESS, HELDOUT, N_KINDS };
    int kind;
    int i[4];     // TRAIN: ls, stage_local, mode, fold_mask | ADAM: ls, fold, tail_a, fold_mask |
                  // FINALIZE: mask | others: 0
    int peer;     // ADAM: 1 = takes the peer's exchange arguments, | 2 = wx, | 4 = afold
    int par;      // parity of the buffers the round writes, (r + 1) & 1 (peer arguments, late fold)
    FLSel p[5];   // buffer arguments in launcher order
};
// The same kernel with the same scalar arguments / the same buffer arguments.
inline bool same_launch(const FLLaunchRec& a, const FLLaunchRec& b) {
    if (a.kind != b.kind || a.peer != b.peer || a.par != b.par) return false;
    for (int k = 0; k < 4; ++k)
        if (a.i[k] != b.i[k]) return false;
    return true;
}
inline bool same_buffers(const FLLaunchRec& a, const FLLaunchRec& b) {
    for (int k = 0; k < 5; ++k)
        if (!(a.p[k] == b.p[k])) return false;
    return true;
}

// Launches of one planning call: fixed capacity, nothing allocated per round.  A round holds at
// most 2 * local_steps + 6 records (flush, pack, the train/Adam pairs, DP or compression, eval, all-reduce,
// server, held-out), so engines take at most FL_PLAN_MAX_LOCAL_STEPS = 61 local steps
// (fedmi/fl/engine.py MAX_LOCAL_STEPS states the same number).
#define FL_PLAN_CAP 128
#define FL_PLAN_MAX_LOCAL_STEPS ((FL_PLAN_CAP - 5) / 2)
struct RoundPlan {
    int n = 0;
    FLLaunchRec rec[FL_PLAN_CAP];
    void push(int kind, int i0, int i1, int i2, int i3, int par, FLSel p0, FLSel p1 = {-1, 0, 0},
              FLSel p2 = {-1, 0, 0}, FLSel p3 = {-1, 0, 0}, FLSel p4 = {-1, 0, 0}, int peer = 0) {
        if (n >= FL_PLAN_CAP) throw std::runtime_error("round plan: too many launches for one call");
        rec[n++] = FLLaunchRec{kind, {i0, i1, i2, i3}, peer, par, {p0, p1, p2, p3, p4}};
    }
    const FLLaunchRec* begin() const { return rec; }
    const FLLaunchRec* end() const { return rec + n; }
};

// What is fixed after construction / attach_peer.
struct RoundTraits {
    int dtype = 0;        // 0 = fp32, 1 = bf16 kernels
    int world = 1;
    int local_steps = 1;
    long long cm_off = 0; // bytes from a parameter buffer to this rank's confusion slots in its tail
    bool es_enabled = false;
    bool fused = false;   // rounds evaluate the previous round inside the train kernel
    bool lag_ok = false;  // lagged rounds possible (layout, clients, bf16): see lagged()
    bool xchg = false;    // lagged rounds: FedAvg inside the Adam kernel (no all-reduce kernel)
    bool has_peer = false;
    bool emulate = false; // one process stands in for a multi-client round (measurements, tests)
    bool dp_on = false;
    bool compress_on = false;  // never with dp_on
    bool server_on = false;
    bool eval_fedavg_fits = false;
    bool identity = false;  // FedAvg is the identity: world == 1 && agg_scale == 1
    // Held-out scoring (fl_heldout.hip): every round the engine aggregates ends with a HELDOUT record on
    // its output image.  A round that a late fold may still discard must not leave a history row (or
    // take the best image) behind, so no rounds are lagged while it is on -- as with a foreign output.
    bool heldout_on = false;

    // Lagged rounds: allowed by the layout, and either no early stopping (metrics may be
    // folded one round late), the Adam-fused exchange (which folds them in time) or an
    // external all-reduce (RCCL: folded one round late, a round run past a stop is discarded
    // bit-exactly -- late_fold()).  A peer all-reduce kernel without the in-kernel exchange
    // (several local steps) keeps classic rounds with early stopping: its send buffer is not the
    // output buffer a late stop republishes from.
    bool lagged() const { return lag_ok && !heldout_on && (!es_enabled || xchg || !has_peer); }
    bool late_fold() const { return lagged() && es_enabled && !xchg; }
    // The engine produces round outputs itself: one client, its peer all-reduce, or RCCL.
    bool aggregates(bool comm_present) const { return world < 2 || has_peer || comm_present; }
    // The round's output is not the aggregated local model (DP: the clipped, noised contribution;
    // compression: x + the compressed update; server optimizer: x + a server step), so rounds are
    // classic and always stage a fresh pack.
    bool foreign_output() const { return dp_on || compress_on || server_on; }
};

// Which metrics the last issued round left pending, and the state of the packed bf16 image.
struct RoundCarry {
    bool pending_cm = false;  // the last issued round was fused: its metrics are not scored yet
    bool cm_in_tail = false;  // the last round's counts sit in the tail, not yet folded
    bool prev_lagged = false; // the last issued round had no evaluation of its own
    bool prev_scored = false; // the last issued round's train kernel scored its predecessor
    bool prev_afold = false;  // ... and its Adam kernel folded that predecessor (exchanged in-kernel)
    bool need_pack = true;    // host changed the global weights: repack before the next round
    bool srv_packed = false;  // bf16: pk_global holds the last server step's output (nothing ran since)

    // (bits 1..32 are stored and restored by callers that capture rounds into graphs of their own)
    int bits() const {
        return (pending_cm ? 1 : 0) | (cm_in_tail ? 2 : 0) | (prev_lagged ? 4 : 0) | (prev_scored ? 8 : 0) |
               (prev_afold ? 16 : 0) | (need_pack ? 32 : 0) | (srv_packed ? 64 : 0);
    }
    static RoundCarry from_bits(int f) {
        RoundCarry c;
        c.pending_cm = f & 1;
        c.cm_in_tail = f & 2;
        c.prev_lagged = f & 4;
        c.prev_scored = f & 8;
        c.prev_afold = f & 16;
        c.need_pack = f & 32;
        c.srv_packed = f & 64;
        return c;
    }
    // The carry with the metric state `m`'s and its own pack state.
    RoundCarry with_metrics_of(const RoundCarry& m) const {
        RoundCarry c = m;
        c.need_pack = need_pack;
        c.srv_packed = srv_packed;
        return c;
    }
    // After a replayed graph of this engine's steady round kind.
    RoundCarry steady(const RoundTraits& t) const {
        RoundCarry m;
        m.pending_cm = t.fused;
        m.cm_in_tail = !t.fused;
        m.prev_lagged = m.prev_scored = t.lagged();
        m.prev_afold = t.lagged() && t.xchg;
        return with_metrics_of(m);
    }
    // The host loaded a complete round state (resume): no metrics are pending.
    RoundCarry cleared() const { return with_metrics_of(RoundCarry{}); }
};

// The captured rounds assume the steady state of their kind: a fused graph must not
// start behind a classic round (whose counts already sit in the tail), a classic graph
// not behind a fused one (whose counts were never computed).
// A lagged graph must start behind a lagged round that scored ITS predecessor: the first
// captured round's fold mask (region A of the round before) is fixed at capture, and every
// replay after the first starts behind such a round.  (Captured behind a lagged round that
// followed a self-evaluating one -- e.g. a warm-up that closed on an odd round count -- every
// replay's first round skipped the region-A fold: that round's metrics never reached the
// history or the early-stop rule.  The Adam-fused exchange folds in time and was unaffected.)
inline bool needs_eager_round(const RoundTraits& t, const RoundCarry& c) {
    if (t.lagged()) return !c.prev_lagged || !c.prev_scored;
    return t.fused ? c.cm_in_tail : c.pending_cm;
}

inline FLSel fl_at(int base, long long off = 0) { return FLSel{base, 0, off}; }
// Buffer a round of output parity `par` publishes into (FedAvg contribution + metric tails): the
// peer all-reduce's send buffer, or, for RCCL, the parameter buffer it reduces in place.
inline FLSel plan_comm_buf(const RoundTraits& t, int par) {
    return fl_at((t.has_peer ? FL_TB_COMM0 : FL_TB_PBUF0) + par);
}

inline void plan_eval(const RoundTraits& t, RoundPlan& out, int r) {
    const int par = (r + 1) & 1;
    out.push(FLLaunchRec::EVAL, 0, 0, 0, 0, par, fl_at(FL_TB_LOCAL), plan_comm_buf(t, par), fl_at(FL_TB_ST0 + par));
}
// A fused round r-1 left its metrics pending (they are normally scored by round r's
// train kernel): score them with the eval kernel before anything that needs them.
inline void plan_flush_pending_eval(const RoundTraits& t, RoundCarry& c, RoundPlan& out, int r) {
    if (!c.pending_cm) return;
    plan_eval(t, out, r - 1);
    c.pending_cm = false;
    c.cm_in_tail = true;
}

// One train launch, preceded on the bf16 path by the pack of the round's input weights when no
// kernel left their packed image behind.
inline void plan_train_launch(const RoundTraits& t, RoundCarry& c, RoundPlan& out, int par, FLSel pg, FLSel si,
                              FLSel so, int ls, int mode = FL_EVAL_CLASSIC, FLSel cm_out = {-1, 0, 0},
                              int fold_mask = FL_FOLD_B) {
    // (the fp32 kernels read the fp32 image directly: nothing to repack, but need_pack also tells
    // plan_train that the host replaced the weights -- consumed here, or every fused round would
    // flush a separate evaluation)
    bool solo = false;
    if (t.dtype == 1) {
        // With one client the FedAvg output IS the local model (agg_scale = 1), which the Adam
        // kernel already packed, so the pack is needed only after host-side weight changes; later
        // local steps stage the Adam-packed local image too.  Not with a foreign output: DP packs
        // from the fp32 image every round, a server step packs the new global image itself (then
        // neither the peer all-reduce's pack epilogue nor the Adam-packed local image is the input).
        solo = t.identity && !c.need_pack && !t.foreign_output();
        // the peer all-reduce already wrote the packed image of its output
        const bool packed = t.server_on ? (c.srv_packed && !c.need_pack) : (solo || (t.has_peer && !c.need_pack));
        if (ls == 0) c.srv_packed = false;  // a later step without a server launch in between repacks
        if (ls == 0 && !packed) out.push(FLLaunchRec::PACK, 0, 0, 0, 0, par, pg, fl_at(FL_TB_PKG));
    }
    c.need_pack = false;
    out.push(FLLaunchRec::TRAIN, ls, solo ? 1 : 0, mode, fold_mask, par, pg, si, so, cm_out);
}

// Train/Adam pairs of round r.  Fused rounds (FL_EVAL_FUSED): the first train kernel also scores
// the previous round's model from its own forward pass, and the first Adam kernel folds those
// counts and makes the round's live / stop decision.
// Lagged rounds (FL_EVAL_LAGGED): the train kernel scores the previous round's local model
// iff that round had no evaluation of its own; its fold consumes region A when the previous
// round scored ITS predecessor and region B when the previous round was evaluated.
// `xchg`: this round's FedAvg runs inside its Adam kernel (peer_device.h chunk exchange).
inline void plan_train(const RoundTraits& t, RoundCarry& c, RoundPlan& out, int r, bool fused, bool xchg = false) {
    const int in = r & 1, par = (r + 1) & 1;
    const FLSel pg = fl_at(FL_TB_PBUF0 + in), cb = plan_comm_buf(t, par);
    const FLSel si = fl_at(FL_TB_ST0 + in), so = fl_at(FL_TB_ST0 + par), local = fl_at(FL_TB_LOCAL);
    if (fused && c.need_pack) plan_flush_pending_eval(t, c, out, r);  // host replaced the weights: score the old model
    // Every round's metric fold runs in its first Adam kernel (overlapped with the slab
    // loads; measured: folding at the start of the train kernel cost ~3 us per round), the
    // train kernel trains on the tentative live decision.
    const bool score = !fused && c.prev_lagged;
    int mode = (fused && !c.cm_in_tail) ? FL_EVAL_FUSED : FL_EVAL_FUSED_SKIP;
    if (score) mode = FL_EVAL_LAGGED;
    // metrics of the previous round: region B of its all-reduce (it evaluated itself), or
    // region A one round later (lagged, FedAvg outside Adam); with the Adam-fused exchange
    // a lagged predecessor is folded inside this Adam kernel from the exchanged region A
    const bool afold = score && t.xchg;  // fold the lagged predecessor in this Adam kernel
    const int mask = fused ? FL_FOLD_B
                           : ((c.prev_scored && !c.prev_afold ? FL_FOLD_A : 0) | (c.prev_lagged ? 0 : FL_FOLD_B));
    const FLSel cm_out = score ? fl_at(FL_TB_LAG) : fl_at(FL_TB_PBUF0 + in, t.cm_off);
    for (int ls = 0; ls < t.local_steps; ++ls) {
        const bool first = ls == 0;
        plan_train_launch(t, c, out, par, pg, first ? si : so, so, ls, first ? mode : FL_EVAL_CLASSIC, cm_out, mask);
        if (first)
            out.push(FLLaunchRec::ADAM, ls, 1, score ? 1 : 0, mask, par, pg, pg, cb, si, so,
                     (xchg || afold) ? (1 | (xchg ? 2 : 0) | (afold ? 4 : 0)) : 0);
        else
            out.push(FLLaunchRec::ADAM, ls, 0, 0, FL_FOLD_B, par, local, pg, cb, so);
    }
    // clip + noise of the contribution the last Adam kernel stored (fl_dp.hip); `so` holds
    // the round's live flag and index
    if (t.dp_on) out.push(FLLaunchRec::DP, 0, 0, 0, 0, par, local, pg, cb, so);
    // ... or its compression with error feedback (fl_compress.hip), in the same place
    else if (t.compress_on) out.push(FLLaunchRec::COMPRESS, 0, 0, 0, 0, par, local, pg, cb, so);
    c.pending_cm = fused;
    c.cm_in_tail = false;
    c.prev_scored = score;
    c.prev_afold = afold;
}

inline void plan_allreduce(const RoundTraits& t, RoundPlan& out, int r, bool comm_present) {
    // (one client: FedAvg is the identity; an emulating engine still issues the collective,
    // e.g. a one-rank RCCL all-reduce, so the multi-client round shape runs on one GPU)
    if (t.world < 2 && !t.has_peer && !(t.emulate && comm_present)) return;
    if (!t.has_peer && !comm_present) return;
    const int par = (r + 1) & 1;
    out.push(FLLaunchRec::ALLREDUCE, 0, 0, 0, 0, par, fl_at(FL_TB_PBUF0 + par));
}
// Server-optimizer step of round r (fl_server.hip) on the aggregated image in the round's output
// buffer, whose state holds the round's live flag and index.  bf16: also packs the result.
inline void plan_server(const RoundTraits& t, RoundCarry& c, RoundPlan& out, int r) {
    if (!t.server_on) return;
    const int par = (r + 1) & 1;
    out.push(FLLaunchRec::SERVER, 0, 0, 0, 0, par, fl_at(FL_TB_PBUF0 + (r & 1)), fl_at(FL_TB_PBUF0 + par),
             fl_at(FL_TB_ST0 + par));
    c.srv_packed = t.dtype == 1;
}

// Held-out record of round r (fl_heldout.hip): scores the round's finished output image -- aggregated,
// after any server step -- under the round's state (live flag and index), both of the output parity.
inline void plan_heldout(const RoundTraits& t, RoundPlan& out, int r) {
    if (!t.heldout_on) return;
    const int par = (r + 1) & 1;
    out.push(FLLaunchRec::HELDOUT, 0, 0, 0, 0, par, fl_at(FL_TB_PBUF0 + par), fl_at(FL_TB_ST0 + par));
}

// `lag`: a lagged round -- no evaluation; the next round's train kernel scores it.
// `server`: the round ends with the engine's own steps on the aggregated image -- the server-optimizer
// step, then the held-out record (neither when the caller aggregates).
inline void plan_round(const RoundTraits& t, RoundCarry& c, RoundPlan& out, int r, bool allow_fused, bool lag,
                       bool server, bool comm_present) {
    const bool held = server && t.heldout_on && t.aggregates(comm_present);
    server = server && t.server_on && t.aggregates(comm_present);
    const bool fused = t.fused && allow_fused;
    lag = lag && t.lagged() && !fused;
    if (!fused) plan_flush_pending_eval(t, c, out, r);
    const bool xchg = lag && t.xchg;
    plan_train(t, c, out, r, fused, xchg);
    c.prev_lagged = lag;
    if (lag) {
        if (!xchg) plan_allreduce(t, out, r, comm_present);
        return;  // (never with held-out scoring: lagged() is false then)
    }
    if (!fused && t.has_peer && t.eval_fedavg_fits) {
        // evaluation and the one-shot all-reduce in one kernel (peer_device.h)
        const int par = (r + 1) & 1;
        out.push(FLLaunchRec::EVAL_FEDAVG, 0, 0, 0, 0, par, fl_at(FL_TB_LOCAL), plan_comm_buf(t, par),
                 fl_at(FL_TB_ST0 + par));
        c.cm_in_tail = true;
        if (server) plan_server(t, c, out, r);
        if (held) plan_heldout(t, out, r);
        return;
    }
    if (!fused) {
        plan_eval(t, out, r);
        c.cm_in_tail = true;
    }
    plan_allreduce(t, out, r, comm_present);
    if (server) plan_server(t, c, out, r);
    if (held) plan_heldout(t, out, r);
}

// One phase of round r: 0 = local training (all local steps), 1 = local evaluation,
// 2 = FedAvg all-reduce (+ the server-optimizer step and the held-out record when the engine
// aggregates itself), 3 = the server-optimizer step alone, 4 = the held-out record alone (the caller
// aggregated the round's buffer; 4 after 3).  Always classic rounds.
inline void plan_phase(const RoundTraits& t, RoundCarry& c, RoundPlan& out, int r, int which, bool comm_present) {
    if (which == 0) {
        plan_flush_pending_eval(t, c, out, r);
        plan_train(t, c, out, r, false);
        c.prev_lagged = false;
    } else if (which == 1) {
        plan_eval(t, out, r);
        c.cm_in_tail = true;
    } else if (which == 2) {
        plan_allreduce(t, out, r, comm_present);
        if (t.aggregates(comm_present)) {
            plan_server(t, c, out, r);
            plan_heldout(t, out, r);
        }
    } else if (which == 3) {
        if (!t.server_on) throw std::runtime_error("phase 3: no server optimizer");
        plan_server(t, c, out, r);
    } else if (which == 4) {
        if (!t.heldout_on) throw std::runtime_error("phase 4: no held-out set");
        plan_heldout(t, out, r);
    } else {
        throw std::runtime_error("phase: 0, 1, 2, 3 or 4");
    }
}

// Fold every pending metric into the state / history; `r` = rounds issued.  A fused last round
// is evaluated first.
inline void plan_finalize(const RoundTraits& t, RoundCarry& c, RoundPlan& out, int r) {
    plan_flush_pending_eval(t, c, out, r);
    if (c.prev_lagged)
        throw std::runtime_error("finalize: the last round is lagged (its metrics need one more round)");
    const int mask = (c.prev_scored && !c.prev_afold ? FL_FOLD_A : 0) | FL_FOLD_B;
    const int in = r & 1, par = (r + 1) & 1;
    out.push(FLLaunchRec::FINALIZE, mask, 0, 0, 0, par, fl_at(FL_TB_PBUF0 + in), fl_at(FL_TB_ST0 + in),
             fl_at(FL_TB_ST0 + par));
    c.cm_in_tail = false;
}
