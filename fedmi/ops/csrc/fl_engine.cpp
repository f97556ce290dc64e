// Native runtime of the federated round engine: kernel sequencing, HIP-graph capture of
// whole rounds, and an RCCL communicator owned by the engine (no torch / pickle in the
// round loop).  Exposed to Python as module `fedmi.ops._fedmi_hip` (pybind11).
//
// The reference runs the round loop in Python with 3 gathers + 3 bcasts + (2 + 2k)
// barriers per round (FL_CustomMLPCLassifierImplementation_Multiple_Rounds.py:130-201,
// SURVEY §2.4).  Here `FLEngine::run` issues, per round, three kernels and one
// ncclAllReduce on the caller's stream; `capture` records an even number of rounds into a
// hipGraph that is replayed with one host call.  Early stopping is decided on the device,
// so nothing in the loop waits on the host.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <cmath>
#include <thread>
#include <vector>

#include "fl_common.h"
#include "fl_layout.h"
#include "fl_round_plan.h"
#include "peer_allreduce.h"

namespace py = pybind11;

#define HIP_CHECK(expr)                                                                       \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(_e) +     \
                                     " at " #expr);                                           \
    } while (0)

#define NCCL_CHECK(expr)                                                                      \
    do {                                                                                      \
        ncclResult_t _r = (expr);                                                             \
        if (_r != ncclSuccess)                                                                \
            throw std::runtime_error(std::string("RCCL error ") + ncclGetErrorString(_r) +   \
                                     " at " #expr);                                           \
    } while (0)

hipError_t fl_set_lds_limit(size_t bytes);  // fl_kernels.hip
void register_trainer(pybind11::module_& m);  // mlp_trainer.cpp

static inline hipStream_t as_stream(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }
template <typename T>
static inline T* as_ptr(uintptr_t p) { return reinterpret_cast<T*>(p); }

// ---------------------------------------------------------------------------------------
// RCCL communicator: one per process (= one per GPU / federated client).
// ---------------------------------------------------------------------------------------
//
// The communicator is NON-BLOCKING (ncclConfig_t::blocking = 0): ncclCommInitRankConfig returns at
// once and the bootstrap (unique-id rendezvous, topology, rings) runs inside RCCL while this thread
// polls ncclCommGetAsyncError against a deadline with the GIL released.  A peer that never calls
// init (died before it, stuck elsewhere) therefore ends in ncclCommAbort and a Python exception
// naming the deadline, not in a process blocked forever inside ncclCommInitRank -- the reference's
// contract is "any failure -> comm.Abort()" (C:203-205).  Every later call on a non-blocking
// communicator may also return ncclInProgress (e.g. the lazy connection set-up of the first
// collective); `settle` waits those out under the same deadline.
class RcclComm {
  public:
    RcclComm(int nranks, int rank, py::bytes uid, int device, double timeout_s)
        : nranks_(nranks), rank_(rank), timeout_s_(timeout_s) {
        std::string s = uid;
        if (s.size() != sizeof(ncclUniqueId)) throw std::runtime_error("bad RCCL unique id size");
        ncclUniqueId id;
        std::memcpy(&id, s.data(), sizeof(id));
        HIP_CHECK(hipSetDevice(device));
        ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
        cfg.blocking = 0;
        ncclResult_t r;
        {
            py::gil_scoped_release nogil;
            r = ncclCommInitRankConfig(&comm_, nranks, id, rank, &cfg);
            if (r == ncclSuccess || r == ncclInProgress) r = wait_settled();
        }
        if (r != ncclSuccess) {
            if (comm_) {
                py::gil_scoped_release nogil;
                ncclCommAbort(comm_);
            }
            comm_ = nullptr;
            if (r == ncclInProgress)
                throw std::runtime_error("RCCL bootstrap timed out after " + std::to_string(timeout_s_) +
                                         " s (rank " + std::to_string(rank) + " of " + std::to_string(nranks) +
                                         "): a peer never joined ncclCommInitRankConfig; communicator aborted");
            throw std::runtime_error(std::string("RCCL bootstrap failed: ") + ncclGetErrorString(r));
        }
    }
    ~RcclComm() { destroy(); }

    static py::bytes unique_id() {
        ncclUniqueId id;
        NCCL_CHECK(ncclGetUniqueId(&id));
        return py::bytes(reinterpret_cast<const char*>(&id), sizeof(id));
    }

    void allreduce_f32(uintptr_t buf, size_t count, uintptr_t stream) {
        settle(ncclAllReduce(as_ptr<float>(buf), as_ptr<float>(buf), count, ncclFloat32, ncclSum, live(),
                             as_stream(stream)), "ncclAllReduce(f32)");
    }
    void allreduce_bf16(uintptr_t buf, size_t count, uintptr_t stream) {
        settle(ncclAllReduce(as_ptr<void>(buf), as_ptr<void>(buf), count, ncclBfloat16, ncclSum, live(),
                             as_stream(stream)), "ncclAllReduce(bf16)");
    }
    void allreduce_f64(uintptr_t buf, size_t count, uintptr_t stream) {
        settle(ncclAllReduce(as_ptr<double>(buf), as_ptr<double>(buf), count, ncclFloat64, ncclSum, live(),
                             as_stream(stream)), "ncclAllReduce(f64)");
    }
    void broadcast_bytes(uintptr_t buf, size_t nbytes, int root, uintptr_t stream) {
        settle(ncclBroadcast(as_ptr<void>(buf), as_ptr<void>(buf), nbytes, ncclUint8, root, live(),
                             as_stream(stream)), "ncclBroadcast");
    }
    void allgather_f32(uintptr_t send, uintptr_t recv, size_t count, uintptr_t stream) {
        settle(ncclAllGather(as_ptr<float>(send), as_ptr<float>(recv), count, ncclFloat32, live(),
                             as_stream(stream)), "ncclAllGather");
    }
    // ncclCommGetAsyncError of a live communicator (0 = ncclSuccess); lets a watchdog see an
    // asynchronous RCCL failure without issuing a collective.
    int async_error() const {
        if (!comm_) return (int)ncclInvalidArgument;
        ncclResult_t st = ncclSuccess;
        ncclCommGetAsyncError(comm_, &st);
        return (int)st;
    }
    void abort() {
        if (comm_) {
            ncclCommAbort(comm_);
            comm_ = nullptr;
        }
    }
    void destroy() {
        if (comm_) {
            ncclCommDestroy(comm_);
            comm_ = nullptr;
        }
    }
    int rank() const { return rank_; }
    int size() const { return nranks_; }
    ncclComm_t handle() const { return comm_; }

  private:
    ncclComm_t live() const {
        if (!comm_) throw std::runtime_error("RCCL communicator used after abort/destroy");
        return comm_;
    }
    // Poll the communicator's state until it leaves ncclInProgress or the deadline passes
    // (returns ncclInProgress then).  Called without the GIL.
    ncclResult_t wait_settled() const {
        const auto t_end = std::chrono::steady_clock::now() +
                           std::chrono::microseconds((long long)(timeout_s_ * 1e6));
        ncclResult_t st = ncclInProgress;
        for (;;) {
            if (ncclCommGetAsyncError(comm_, &st) != ncclSuccess) return ncclInternalError;
            if (st != ncclInProgress) return st;
            if (std::chrono::steady_clock::now() >= t_end) return ncclInProgress;
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
    }
    void settle(ncclResult_t r, const char* what) {
        if (r == ncclInProgress) {
            if (PyGILState_Check()) {
                py::gil_scoped_release nogil;
                r = wait_settled();
            } else {
                r = wait_settled();
            }
        }
        if (r != ncclSuccess)
            throw std::runtime_error(std::string("RCCL error ") +
                                     (r == ncclInProgress ? "timeout" : ncclGetErrorString(r)) + " in " + what);
    }
    int nranks_, rank_;
    double timeout_s_;
    ncclComm_t comm_ = nullptr;
};

// ---------------------------------------------------------------------------------------
// Engine
// ---------------------------------------------------------------------------------------
// Every launch of a round is planned on the host first (fl_round_plan.h: a pure function of the
// engine's RoundTraits and its RoundCarry) and then executed from its record: by this engine
// (execute), or batched over the engines of a trial batch (TrialBatch below).
class TrialBatch;

class FLEngine {
    friend class TrialBatch;

  public:
    FLEngine(std::vector<int> dims, py::dict cfg, py::dict bufs) {
        const int L = (int)dims.size() - 1;
        if (L < 1 || L > FL_MAX_LAYERS) throw std::runtime_error("FLEngine: 1..4 Linear layers supported");
        std::memset(&d_, 0, sizeof(d_));
        std::memset(&c_, 0, sizeof(c_));
        std::memset(&b_, 0, sizeof(b_));
        c_.R = cfg["R"].cast<int>();
        if (c_.R != 16 && c_.R != 32 && c_.R != 64) throw std::runtime_error("FLEngine: R must be 16, 32 or 64");
        const int C = dims[L];
        if (C > FL_MAX_CLASSES) throw std::runtime_error("FLEngine: at most 16 classes");
        if (dims[0] > 4096) throw std::runtime_error("FLEngine: too many features");
        fl_build_fp32_layout(dims.data(), L, c_.R, &d_);   // fl_layout.h (host-tested with sanitizers)
        const int lds = d_.lds_floats;
        dtype_ = cfg.contains("dtype") ? cfg["dtype"].cast<int>() : 0;
        if (dtype_ == 0) {
            if (c_.R == 64) throw std::runtime_error("FLEngine: R = 64 needs the bf16 kernels");
            if ((size_t)lds * 4 > FL_LDS_DYNAMIC_MAX)
                throw std::runtime_error("FLEngine: activations exceed LDS; use a smaller R or the layered path");
            HIP_CHECK(fl_set_lds_limit((size_t)lds * 4));
        } else {
            fl_build_bf16_layout(d_, c_.R, &e_, &ev_);
            // FEDMI_LAG_REG=0: lagged rounds score before the training pass instead of beside it (A/B)
            const char* lreg_env = std::getenv("FEDMI_LAG_REG");
            if (lreg_env != nullptr && lreg_env[0] == '0') e_.lag_reg = ev_.lag_reg = 0;
            const size_t need = (size_t)std::max(e_.lds_bytes, ev_.lds_bytes);
            if (need > FL_LDS_DYNAMIC_MAX)
                throw std::runtime_error("FLEngine(bf16): model exceeds LDS; use a smaller R or the layered path");
            HIP_CHECK(fl_set_lds_limit_bf16(need));
        }

        c_.n_rows = cfg["n_rows"].cast<int>();
        c_.inv_n = 1.0f / (float)c_.n_rows;
        c_.world = cfg["world"].cast<int>();
        c_.rank = cfg["rank"].cast<int>();
        if (c_.world > FL_MAX_WORLD) throw std::runtime_error("FLEngine: world too large");
        c_.agg_scale = cfg["agg_scale"].cast<float>();
        c_.slab_stride = ((d_.P + 1) + 3) & ~3;
        c_.n_slabs = (c_.n_rows + c_.R - 1) / c_.R;
        // bf16 kernels: fp16 gradient partials unless the caller asks for fp32 (engine.py grad_slab)
        c_.slab_f16 = dtype_ == 1 && (cfg.contains("slab_f16") ? cfg["slab_f16"].cast<bool>() : true) ? 1 : 0;
        c_.tail_off = d_.Pimg;
        c_.tail_stride = C * C + 1;
        c_.tail_len = c_.world * c_.tail_stride;
        c_.local_steps = cfg["local_steps"].cast<int>();
        c_.lr0 = cfg["lr"].cast<double>();
        c_.gamma = cfg["gamma"].cast<double>();
        c_.step_size = cfg["step_size"].cast<int>();
        c_.beta1 = cfg["beta1"].cast<double>();
        c_.beta2 = cfg["beta2"].cast<double>();
        c_.omb1 = (float)(1.0 - c_.beta1);
        c_.omb2 = (float)(1.0 - c_.beta2);
        c_.beta2f = (float)c_.beta2;
        c_.eps = (float)cfg["eps"].cast<double>();
        c_.weight_decay = (float)cfg["weight_decay"].cast<double>();
        c_.prox_mu = (float)cfg["prox_mu"].cast<double>();
        c_.es_enabled = cfg["early_stop"].cast<bool>() ? 1 : 0;
        c_.patience = cfg["patience"].cast<int>();
        c_.atol = cfg["atol"].cast<double>();
        c_.rtol = cfg["rtol"].cast<double>();
        c_.max_rounds = cfg["max_rounds"].cast<int>();
        c_.metric_mode = cfg["metric_mode"].cast<int>();
        // ---- round kind (RoundTraits, fl_round_plan.h) ----
        tr_.dtype = dtype_;
        tr_.world = c_.world;
        tr_.local_steps = c_.local_steps;
        if (c_.local_steps > FL_PLAN_MAX_LOCAL_STEPS)
            throw std::runtime_error("FLEngine: at most " + std::to_string(FL_PLAN_MAX_LOCAL_STEPS) + " local steps");
        tr_.es_enabled = c_.es_enabled != 0;
        tr_.identity = c_.world == 1 && c_.agg_scale == 1.0f;
        tr_.cm_off = (long long)(c_.tail_off + c_.rank * c_.tail_stride) * (long long)sizeof(float);
        std::memset(&dp_, 0, sizeof(dp_));
        dp_.clip = cfg.contains("dp_clip") ? cfg["dp_clip"].cast<float>() : 0.f;
        tr_.dp_on = dp_.clip > 0.f;
        std::memset(&cp_, 0, sizeof(cp_));
        cp_.kind = cfg.contains("compress") ? cfg["compress"].cast<int>() : FL_COMPRESS_NONE;
        tr_.compress_on = cp_.kind != FL_COMPRESS_NONE;
        if (tr_.compress_on && tr_.dp_on)
            throw std::runtime_error("FLEngine: compression does not combine with differential privacy");
        std::memset(&sv_, 0, sizeof(sv_));
        sv_.kind = cfg.contains("server_opt") ? cfg["server_opt"].cast<int>() : FL_SERVER_NONE;
        tr_.server_on = sv_.kind != FL_SERVER_NONE;
        // The round's output is not the aggregated local model, so rounds are classic:
        // differential privacy (fl_dp.hip) outputs the clipped, noised contribution, not the local
        // model a fused / lagged round's next train kernel would score and stage, and a discarded
        // late-fold round would have spent noise; compression (fl_compress.hip) outputs x + the compressed
        // update and keeps a residual a discarded round would have consumed; a server optimizer (fl_server.hip) outputs x + (a
        // server step), so a fused round would score the wrong model through the global image and a
        // lagged round's in-Adam exchange would publish an image the step then has to replace.
        const bool classic_only = tr_.foreign_output();
        // Fused evaluation needs the round's input weights to BE the previous round's
        // post-step local model: one client (FedAvg of one is the identity, agg_scale 1).
        tr_.fused = !classic_only && cfg.contains("fused_eval") && cfg["fused_eval"].cast<bool>() && tr_.identity;
        if (tr_.dp_on) {
            const unsigned long long seed = cfg["dp_seed"].cast<unsigned long long>();
            dp_.noise = cfg["dp_noise"].cast<bool>() ? 1 : 0;
            dp_.rank = c_.rank;
            dp_.max_rounds = c_.max_rounds;
            dp_.key0 = (uint32_t)seed;
            dp_.key1 = (uint32_t)(seed >> 32);
            dp_.sigma = as_ptr<const float>(bufs["dp_sigma"].cast<uintptr_t>());
            dp_.norm_hist = as_ptr<float>(bufs["dp_norm"].cast<uintptr_t>());
            if (dp_.sigma == nullptr || dp_.norm_hist == nullptr)
                throw std::runtime_error("FLEngine: DP needs the sigma table and the norm history");
        }
        if (tr_.compress_on) {
            if (cp_.kind < FL_COMPRESS_TOPK || cp_.kind > FL_COMPRESS_RANDK)
                throw std::runtime_error("FLEngine: unknown compressor");
            cp_.P = d_.P;
            cp_.k = cp_.kind == FL_COMPRESS_TOPK || cp_.kind == FL_COMPRESS_RANDK ? cfg["compress_k"].cast<int>() : d_.P;
            if (compress_random()) {
                // the stochastic kinds: words of (compress_seed, round, this client), fl_compress.hip
                const unsigned long long seed = cfg["compress_seed"].cast<unsigned long long>();
                cp_.levels = cp_.kind == FL_COMPRESS_QSGD ? cfg["compress_levels"].cast<int>() : 0;
                cp_.client = c_.rank;
                cp_.key0 = (uint32_t)seed;
                cp_.key1 = (uint32_t)(seed >> 32);
                if (cp_.kind == FL_COMPRESS_QSGD && (cp_.levels < 1 || cp_.levels > FL_COMPRESS_MAX_LEVELS))
                    throw std::runtime_error("FLEngine: compress_levels must be in 1 .. 32767");
            }
            cp_.error_feedback = cfg["error_feedback"].cast<bool>() ? 1 : 0;
            cp_.max_rounds = c_.max_rounds;
            cp_.residual = as_ptr<float>(bufs["compress_residual"].cast<uintptr_t>());
            cp_.stat_hist = as_ptr<float>(bufs["compress_stat"].cast<uintptr_t>());
            if (cp_.k < 1 || cp_.k > d_.P) throw std::runtime_error("FLEngine: compress_k must be in 1 .. P");
            if (cp_.residual == nullptr || cp_.stat_hist == nullptr)
                throw std::runtime_error("FLEngine: compression needs the residual and the statistic history");
            HIP_CHECK(fl_set_lds_limit_compress(d_, cp_.kind));
        }
        if (tr_.server_on) {
            if (sv_.kind < FL_SERVER_SGD || sv_.kind > FL_SERVER_YOGI)
                throw std::runtime_error("FLEngine: unknown server optimizer");
            const double b1 = cfg["server_momentum"].cast<double>(), b2 = cfg["server_beta2"].cast<double>();
            sv_.max_rounds = c_.max_rounds;
            sv_.lr = (float)cfg["server_lr"].cast<double>();
            sv_.b1 = (float)b1;
            sv_.omb1 = (float)(1.0 - b1);
            sv_.b2 = (float)b2;
            sv_.omb2 = (float)(1.0 - b2);
            sv_.tau = (float)cfg["server_tau"].cast<double>();
            sv_.m = as_ptr<float>(bufs["server_m"].cast<uintptr_t>());
            sv_.v = sv_.kind == FL_SERVER_SGD ? nullptr : as_ptr<float>(bufs["server_v"].cast<uintptr_t>());
            if (sv_.m == nullptr || (sv_.kind != FL_SERVER_SGD && sv_.v == nullptr))
                throw std::runtime_error("FLEngine: the server optimizer needs its state buffers");
        }
        // Aggregation rule of a multi-rank engine on the peer plane (peer_select.h): a robust aggregator
        // selects, secure aggregation masks this rank's send buffer and opens -- instead of the sum.
        // Used only once a peer is attached (attach_peer); over RCCL such an engine refuses to aggregate.
        std::memset(&sel_, 0, sizeof(sel_));
        {
            const int robust = cfg.contains("robust") ? cfg["robust"].cast<int>() : 0;
            const bool secagg = cfg.contains("secagg") && cfg["secagg"].cast<bool>();
            if (robust && secagg) throw std::runtime_error("FLEngine: secure aggregation does not combine with a robust rule");
            if (robust && tr_.dp_on)
                throw std::runtime_error("FLEngine: a robust rule does not combine with differential privacy");
            if (robust) {
                if (robust != FL_ROBUST_MEDIAN && robust != FL_ROBUST_TRIMMED)
                    throw std::runtime_error("FLEngine: unknown robust rule");
                sel_.mode = PEER_SELECT_ROBUST;
                sel_.rb.kind = robust;
                sel_.rb.K = c_.world;
                sel_.rb.max_rounds = c_.max_rounds;
                sel_.rb.beta = cfg["trim_ratio"].cast<double>();
            } else if (secagg) {
                const unsigned long long seed = cfg["secagg_seed"].cast<unsigned long long>();
                sel_.mode = PEER_SELECT_OPEN;
                sel_.sa.bits = cfg["secagg_bits"].cast<int>();
                sel_.sa.K = c_.world;
                sel_.sa.first_client = c_.rank;
                sel_.sa.max_rounds = c_.max_rounds;
                sel_.sa.key0 = (uint32_t)seed;
                sel_.sa.key1 = (uint32_t)(seed >> 32);
                sa_clamp_ = as_ptr<uint32_t>(bufs["sa_clamp"].cast<uintptr_t>());
                if (sa_clamp_ == nullptr) throw std::runtime_error("FLEngine: secure aggregation needs the clamp history");
            }
        }
        {
            // The fused evaluation + FedAvg grid (evaluation blocks + all-reduce blocks) must be
            // resident in one wave, which needs two evaluation workgroups per CU (measured: with one
            // per CU the extra blocks spill into a second wave and the fused kernel loses to the
            // separate kernels, tools/round_emulate.py).
            const size_t lds = dtype_ == 0 ? (size_t)d_.lds_floats * 4 : (size_t)ev_.lds_bytes;
            tr_.eval_fedavg_fits = (!cfg.contains("eval_fedavg") || cfg["eval_fedavg"].cast<bool>()) &&
                                   2 * lds <= (size_t)160 * 1024;
        }
        // Lagged evaluation (fl_common.h FL_EVAL_LAGGED): several clients, early stopping off,
        // bf16 kernels, and room in LDS for the second parameter image.  The comm buffer then
        // carries the lag region A after the tails (the caller sized it: comm_len).
        const bool lag_req = !classic_only && cfg.contains("lagged_eval") && cfg["lagged_eval"].cast<bool>();
        if (lag_req) c_.lag_off = d_.Pimg + c_.tail_len;
        comm_len_ = d_.Pimg + c_.tail_len * (lag_req ? 2 : 1);
        const bool emulate = cfg.contains("emulate_clients") && cfg["emulate_clients"].cast<bool>();
        tr_.emulate = emulate;
        // (with early stopping the rounds are lagged when the FedAvg runs inside the Adam kernel,
        // which folds the metrics in time, or rides RCCL, folded one round late: see lagged())
        // (the lagged train kernel scores the previous local model in the train layout itself)
        tr_.lag_ok = lag_req && dtype_ == 1 && (c_.world > 1 || emulate) && !tr_.fused;
        // several clients + register scoring: the training forward pass is plain bf16 (no round
        // scores from it), in every round kind of the engine alike (lagged, classic, step API).
        // cfg["plain_fwd"] (EngineConfig.plain_fwd): -1 auto, 0 off, 1 on wherever valid;
        // FEDMI_PLAIN_FWD=0 forces the split forward (A/B builds)
        {
            const int req = cfg.contains("plain_fwd") ? cfg["plain_fwd"].cast<int>() : -1;
            const char* pf = std::getenv("FEDMI_PLAIN_FWD");
            const bool valid = dtype_ == 1 && e_.lag_reg && !tr_.fused;
            const bool want = req < 0 ? (c_.world > 1 || emulate) : req > 0;
            c_.plain_fwd = (valid && want && !(pf != nullptr && pf[0] == '0')) ? 1 : 0;
        }
        // split scoring: with register scoring (e_.lag_reg) and a train grid that leaves at least as
        // many CUs idle as it occupies, lagged rounds score on workgroups of their own (the shards
        // of 4-8 clients); FEDMI_SPLIT_SCORE=0 / 1 forces it off / on (A/B)
        {
            int cus = 0, dev = 0;
            if (hipGetDevice(&dev) != hipSuccess ||
                hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
                cus = 0;
            const char* ss = std::getenv("FEDMI_SPLIT_SCORE");
            const bool force_on = ss != nullptr && ss[0] == '1', force_off = ss != nullptr && ss[0] == '0';
            c_.split_score = (tr_.lag_ok && dtype_ == 1 && e_.lag_reg && !force_off &&
                              (force_on || 2 * c_.n_slabs <= cus)) ? 1 : 0;
        }

        // shape-specialised train kernels (fl_train_bf16_spec.hip, fl_train_spec.hip): on by default, FEDMI_SHAPE_SPEC=0
        // forces the generic kernels (A/B, tests).  The launch function decides per launch; reported
        // as layout()["shape_spec"]: the one-client round's train kernel is the specialised one
        {
            const char* sp = std::getenv("FEDMI_SHAPE_SPEC");
            shape_spec_on_ = !(sp != nullptr && sp[0] == '0');
            // the Adam kernel of the same shape (fl_adam_spec.hip): under the same switch, and
            // FEDMI_ADAM_SPEC=0 turns it off alone; reported as layout()["adam_spec"]
            const char* ap = std::getenv("FEDMI_ADAM_SPEC");
            adam_spec_on_ = shape_spec_on_ && !(ap != nullptr && ap[0] == '0');
        }

        b_.X = as_ptr<const float>(bufs["X"].cast<uintptr_t>());
        b_.y = as_ptr<const int>(bufs["y"].cast<uintptr_t>());
        b_.slab = as_ptr<float>(bufs["slab"].cast<uintptr_t>());
        b_.local = as_ptr<float>(bufs["local"].cast<uintptr_t>());
        b_.m = as_ptr<float>(bufs["m"].cast<uintptr_t>());
        b_.v = as_ptr<float>(bufs["v"].cast<uintptr_t>());
        b_.hist_global = as_ptr<double>(bufs["hist_global"].cast<uintptr_t>());
        b_.hist_rank = as_ptr<double>(bufs["hist_rank"].cast<uintptr_t>());
        b_.hist_loss = as_ptr<float>(bufs["hist_loss"].cast<uintptr_t>());
        pbuf_[0] = as_ptr<float>(bufs["params0"].cast<uintptr_t>());
        pbuf_[1] = as_ptr<float>(bufs["params1"].cast<uintptr_t>());
        st_[0] = as_ptr<FLState>(bufs["state0"].cast<uintptr_t>());
        st_[1] = as_ptr<FLState>(bufs["state1"].cast<uintptr_t>());
        // Adam/StepLR schedule and per-round FedAvg table (fl_common.h FLBuffers::sched / rtab):
        // host-built device tables owned by the caller
        b_.sched = as_ptr<const float>(bufs["sched"].cast<uintptr_t>());
        b_.rtab = as_ptr<const float>(bufs["rtab"].cast<uintptr_t>());
        b_.sat = bufs.contains("sat") ? as_ptr<int>(bufs["sat"].cast<uintptr_t>()) : nullptr;
        {
            // FL_EVAL_LAGGED: previous round's counts + loss (zero)
            const size_t nlag = FL_MAX_CLASSES * FL_MAX_CLASSES + 4;
            HIP_CHECK(hipMalloc(&lagbuf_, nlag * sizeof(float)));
            HIP_CHECK(hipMemset(lagbuf_, 0, nlag * sizeof(float)));
            b_.cnt = lagbuf_;
            b_.lbuf = lagbuf_ + FL_MAX_CLASSES * FL_MAX_CLASSES;
        }
        if (dtype_ == 1) {
            // packed bf16 parameter regions; padding stays zero forever
            HIP_CHECK(hipMalloc(&pk_, 2 * (size_t)e_.param_bytes));
            HIP_CHECK(hipMemset(pk_, 0, 2 * (size_t)e_.param_bytes));
            b_.pk_global = pk_;
            b_.pk_local = pk_ + e_.param_bytes;
        }
        if (tr_.lag_ok && c_.es_enabled) {
            // pre-round [local | m | v | packed local image] for a round a late fold discards
            // (FLBuffers::undo); used only while late_fold() (refresh_undo)
            if ((e_.param_bytes & 3) != 0 || (d_.Pimg & 3) != 0)
                throw std::runtime_error("undo buffer: image sizes must be multiples of 4");
            const size_t bytes = 3 * (size_t)d_.Pimg * sizeof(float) + (dtype_ == 1 ? (size_t)e_.param_bytes : 0);
            HIP_CHECK(hipMalloc(&undo_, bytes));
            HIP_CHECK(hipMemset(undo_, 0, bytes));
            b_.undo_pk_bytes = dtype_ == 1 ? e_.param_bytes : 0;
        }
        refresh_undo();
        fill_bases();
        // Blocked fp16 slab row (fl_layout.h FlSlabBlk), reported as layout()["slab_blocked"]: every train
        // launch of this engine takes the specialised bf16 kernel (no lagged rounds, hence every mode
        // fl_train_bf16_spec_ok accepts), every Adam launch the specialised Adam kernel, the slab is
        // fp16, and the caller sized the slab for the longer row (bufs["slab_floats"]) and did not opt
        // out (cfg["slab_blocked"]: engines of a trial batch keep the dense row of the batch kernels).
        // Both launchers get the flag with every launch and refuse any other kernel under it.
        // FEDMI_SLAB_BLOCKED=0 keeps the dense row under the same kernels (A/B, tests).
        {
            const char* sbe = std::getenv("FEDMI_SLAB_BLOCKED");
            const bool want = (!cfg.contains("slab_blocked") || cfg["slab_blocked"].cast<bool>()) &&
                              !(sbe != nullptr && sbe[0] == '0');
            const long long have = bufs.contains("slab_floats") ? bufs["slab_floats"].cast<long long>() : 0;
            const int stride = ((FlRefSlabBlk<32>::s.P + 1) + 3) & ~3;
            slab_blocked_ = want && dtype_ == 1 && c_.slab_f16 && shape_spec_on_ && !tr_.lag_ok &&
                            fl_train_bf16_spec_ok(d_, e_, c_, FL_EVAL_FUSED) && adam_spec_ok() &&
                            have >= (long long)c_.n_slabs * stride;
#ifdef FL_ADAM_GENERAL_ONLY
            slab_blocked_ = false;
#endif
            if (slab_blocked_) c_.slab_stride = stride;
        }
        // Exchanged epilogues of the specialised bf16 train kernel (fl_layout.h fl_epi_*), reported as
        // layout()["epi_exchange"]: on wherever that kernel runs.  FEDMI_EPI_EXCHANGE=0 keeps the generic
        // epilogues under the same kernel (A/B, tests).  The launcher gets the flag with every launch.
        {
            const char* ee = std::getenv("FEDMI_EPI_EXCHANGE");
            epi_exchange_ = !(ee != nullptr && ee[0] == '0') && dtype_ == 1 && shape_spec_on_ &&
                            fl_train_bf16_spec_ok(d_, e_, c_, FL_EVAL_FUSED);
        }
    }

    ~FLEngine() {
        drop_graph();
        if (undo_) (void)hipFree(undo_);
        if (sa_tab_) (void)hipFree(sa_tab_);
        if (pk_) (void)hipFree(pk_);
        if (lagbuf_) (void)hipFree(lagbuf_);
    }

    // Issue rounds [r0, r0 + n): per round the train/Adam pair (one per local step), the
    // evaluation (classic rounds) and, when world > 1, one all-reduce.
    // Lagged engines (several clients, no early stop) issue every round lagged except, with
    // `close`, the last, which evaluates itself: after it every metric is in the buffers.
    void run(int r0, int n, uintptr_t stream, RcclComm* comm, bool close = true) {
        hipStream_t s = as_stream(stream);
        for (int r = r0; r < r0 + n; ++r) issue_round(r, s, comm, lagged() && !(close && r == r0 + n - 1));
    }

    // Local part of round r (no all-reduce; the caller reduces a shared buffer -- and, on a
    // server-optimizer engine, issues phase 3 once the sum is in this engine's buffer).
    void run_local(int r, uintptr_t stream) {
        issue([&](RoundPlan& p) { plan_round(tr_, carry_, p, r, false, false, false, false); }, as_stream(stream),
              nullptr);
    }

    // One phase of round r (plan_phase); used by the step-by-step reference API
    // (train_one_epoch / evaluate_local / federated_averaging).
    void phase(int r, int which, uintptr_t stream, RcclComm* comm) {
        issue([&](RoundPlan& p) { plan_phase(tr_, carry_, p, r, which, comm != nullptr); }, as_stream(stream), comm);
    }

    // Fold every pending metric into the state / history (host synchronisation point); `r`
    // = rounds issued.  A fused last round is evaluated first.
    void finalize(int r, uintptr_t stream) {
        issue([&](RoundPlan& p) { plan_finalize(tr_, carry_, p, r); }, as_stream(stream), nullptr);
    }

    // Record `n` rounds (n even, starting at an even round) into one hipGraph.  Round
    // indices live on the device, so the same graph is replayed for every chunk.  A graph
    // always starts from the steady state (see needs_eager_round).
    //
    // Captured graphs are cached by round count (up to kMaxGraphs): callers that alternate
    // between graph lengths (run() at cfg.graph_rounds, the streaming console's shorter chunks
    // of lagged engines) select the instantiated graph again instead of re-capturing it (ADVICE
    // r4).  A graph is a pure function of the engine's configuration and buffers -- every change
    // of those drops the cache (drop_graph) -- except a pending repack of host-written weights
    // (RoundCarry::need_pack), which is captured into the graph's first round: with one pending the
    // graph is captured afresh.
    void capture(int n, uintptr_t stream, RcclComm* comm) {
        if (n <= 0 || (n & 1)) throw std::runtime_error("capture: n must be a positive even number");
        if (needs_eager_round()) throw std::runtime_error("capture: issue one eager round first");
        for (size_t i = 0; i < graphs_.size(); ++i)
            if (graphs_[i].n == n) {
                if (!carry_.need_pack && graphs_[i].comm == comm) {
                    select_graph((int)i);
                    return;
                }
                destroy_rec(graphs_[i]);
                graphs_.erase(graphs_.begin() + i);
                break;
            }
        if ((int)graphs_.size() >= kMaxGraphs) {
            destroy_rec(graphs_.front());
            graphs_.erase(graphs_.begin());
        }
        graph_ = nullptr;
        exec_ = nullptr;
        hipStream_t s = as_stream(stream);
        const RoundCarry carry0 = carry_;
        const long long ev0 = eval_launches_;
        HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        try {
            for (int r = 0; r < n; ++r) issue_round(r, s, comm, lagged());
        } catch (...) {
            hipGraph_t g;
            hipStreamEndCapture(s, &g);
            if (g) hipGraphDestroy(g);
            carry_ = carry0;  // nothing was captured: a pending repack stays pending
            eval_launches_ = ev0;
            throw;
        }
        GraphRec rec{n, nullptr, nullptr, eval_launches_ - ev0 /* counted per replay, not at capture */, comm};
        HIP_CHECK(hipStreamEndCapture(s, &rec.g));
        if (hipGraphInstantiate(&rec.e, rec.g, nullptr, nullptr, 0) != hipSuccess) {
            hipGraphDestroy(rec.g);
            throw std::runtime_error("capture: hipGraphInstantiate failed");
        }
        graphs_.push_back(rec);
        ++captures_;
        select_graph((int)graphs_.size() - 1);
        eval_launches_ = ev0;
        // nothing ran yet: replay() applies the rounds' effect on the metrics; the pack state stays
        // as the captured rounds left it (a pending repack went into the graph's first round)
        carry_ = carry_.with_metrics_of(carry0);
    }

    void replay(uintptr_t stream) {
        if (!exec_) throw std::runtime_error("replay: no captured graph");
        if (needs_eager_round()) throw std::runtime_error("replay: issue one eager round first");
        HIP_CHECK(hipGraphLaunch(exec_, as_stream(stream)));
        eval_launches_ += graph_evals_;
        carry_ = carry_.steady(tr_);
    }

    int graph_rounds() const { return graph_rounds_; }
    long long graph_captures() const { return captures_; }
    // Stand-alone evaluation kernels issued so far (eager launches + every graph replay's):
    // a one-client fused run launches one per host-side weight change / run end, not per round.
    long long eval_launches() const { return eval_launches_; }

    // Host-side round bookkeeping (which metrics the last issued round left pending) as a bit
    // set.  A caller that captures rounds of this engine into its own graph (a trial group)
    // reads it after the capture and restores it after every replay of that graph.
    int flags() const { return carry_.bits(); }
    void set_flags(int f) { carry_ = RoundCarry::from_bits(f); }

    // A graph must start from the steady state of its round kind (fl_round_plan.h).
    bool needs_eager_round() const { return ::needs_eager_round(tr_, carry_); }
    bool lagged() const { return tr_.lagged(); }
    bool late_fold() const { return tr_.late_fold(); }
    // The kernels keep / restore the pre-round state only where a round can be discarded.
    void refresh_undo() { b_.undo = (late_fold() && undo_ != nullptr) ? undo_ : nullptr; }
    bool adam_exchange() const { return tr_.xchg; }
    bool fused() const { return tr_.fused; }

    // Early-stop parameters (train_and_evaluate(termination_patience, tolerance), C:122): the
    // kernels take FLConfig by value, so a captured graph is dropped; the caller rewrites the
    // round state's patience counter before the first round.
    void set_early_stop(int patience, double atol, double rtol) {
        if (patience < 1) throw std::runtime_error("set_early_stop: patience must be >= 1");
        c_.patience = patience;
        c_.atol = atol;
        c_.rtol = rtol;
        drop_graph();
    }

    // Noise key of a DP engine (resume: the checkpoint's stream continues); a kernel argument, so
    // captured graphs are dropped.
    void set_dp_seed(unsigned long long seed) {
        if (!tr_.dp_on) throw std::runtime_error("set_dp_seed: differential privacy is off");
        dp_.key0 = (uint32_t)seed;
        dp_.key1 = (uint32_t)(seed >> 32);
        drop_graph();
    }

    // Philox key of a stochastic compressor (resume: the checkpoint's stream continues); a kernel
    // argument, so captured graphs are dropped.
    void set_compress_seed(unsigned long long seed) {
        if (!compress_random()) throw std::runtime_error("set_compress_seed: no stochastic compressor (qsgd, randk)");
        cp_.key0 = (uint32_t)seed;
        cp_.key1 = (uint32_t)(seed >> 32);
        drop_graph();
    }

    // bf16 engines: the packed split-bf16 image of the round's input weights as the train kernel
    // stages it (param_bytes; tests compare the server step's pack with the stand-alone one)
    py::bytes packed_global(uintptr_t stream) const {
        if (dtype_ != 1) throw std::runtime_error("packed_global: bf16 engines only");
        HIP_CHECK(hipStreamSynchronize(as_stream(stream)));
        std::string out((size_t)e_.param_bytes, '\0');
        HIP_CHECK(hipMemcpy(out.data(), b_.pk_global, out.size(), hipMemcpyDeviceToHost));
        return py::bytes(out);
    }

    // ... and the packed image of the LOCAL model, which the Adam kernel writes beside the fp32
    // step and a one-client round stages instead of packing its input again (plan_train_launch:
    // solo).  A copy-out like packed_global; tests compare it with the stand-alone pack.
    py::bytes packed_local(uintptr_t stream) const {
        if (dtype_ != 1) throw std::runtime_error("packed_local: bf16 engines only");
        HIP_CHECK(hipStreamSynchronize(as_stream(stream)));
        std::string out((size_t)e_.param_bytes, '\0');
        HIP_CHECK(hipMemcpy(out.data(), b_.pk_local, out.size(), hipMemcpyDeviceToHost));
        return py::bytes(out);
    }

    // The host wrote the global weights (set_weights / resume): the next round repacks them.
    void invalidate() { carry_.need_pack = true; }

    // The host loaded a complete round state (resume): no metrics are pending.
    void reset_pending() { carry_ = carry_.cleared(); }

    // Aggregate with the one-shot xGMI all-reduce (peer_allreduce.hip) instead of RCCL: every
    // round publishes into the peer object's send buffers, and its kernel writes the reduced
    // image into this engine's parameter buffer (plus, in bf16 mode, the packed bf16 image).
    void attach_peer(PeerAllReduce& p) {
        // (world 1 is accepted: a one-rank "all-reduce" emulates the multi-client round on
        // one GPU for measurements, tools/round_emulate.py)
        if (tr_.fused || p.world() != c_.world || p.rank() != c_.rank || !p.is_open())
            throw std::runtime_error("attach_peer: communicator does not match this engine");
        if (p.n_floats() != comm_len_)
            throw std::runtime_error("attach_peer: buffer length != parameter image + tails");
        if (sel_.mode != 0 && (p.n_chunks() != 0 || tr_.lag_ok))
            throw std::runtime_error("attach_peer: a selecting engine runs classic rounds on a communicator without "
                                     "chunk flags");
        drop_graph();
        peer_ = &p;
        tr_.has_peer = true;
        slab_blocked_ = false;  // the Adam kernel of an engine with a peer is a generic one: dense rows (same stride)
        if (sel_.mode != 0) {
            // gather-select rounds are classic: train/Adam pairs, the optional DP or compression
            // launch, the evaluation, then the ALLREDUCE record (select / mask + open) and the optional
            // server step -- no fused evaluation + FedAvg kernel, which sums
            tr_.eval_fedavg_fits = false;
            sel_.d = d_;
            sel_.rb.rtab = sel_.sa.rtab = b_.rtab;
            if (sel_.mode == PEER_SELECT_OPEN) {
                // device pointer tables of the mask launch: this rank's two send buffers, its clamp history
                if (sa_tab_ == nullptr) HIP_CHECK(hipMalloc(&sa_tab_, 3 * sizeof(void*)));
                void* tab[3] = {p.send(0), p.send(1), sa_clamp_};
                HIP_CHECK(hipMemcpy(sa_tab_, tab, sizeof(tab), hipMemcpyHostToDevice));
            }
        }
        fill_bases();
        p.prepare_eval((c_.n_rows + c_.R - 1) / c_.R);
        // lagged rounds reduce inside the Adam kernel when the communicator has a chunk-flag
        // table for every Adam block (+ the tail block); one local step per round
        // (chunks: every Adam block, the tail block and the early lag-region chunk)
        tr_.xchg = tr_.lag_ok && c_.local_steps == 1 && p.n_chunks() >= (d_.P + 63) / 64 + 2;
        refresh_undo();
        std::memset(&pp_, 0, sizeof(pp_));
        if (dtype_ == 1) {
            pp_.pk = b_.pk_global;
            pp_.wlo_delta = e_.wlo_delta;
            pp_.pk_wgap = e_.wgap;
            pp_.pk_wxor = e_.wxor;
            pp_.L = d_.L;
            for (int l = 0; l < d_.L; ++l) {
                const int K = d_.dim[l], N = d_.dim[l + 1];
                pp_.img4_w[l] = d_.iw_off[l] / 4;
                pp_.img4_b[l] = d_.ib_off[l] / 4;
                pp_.img4_end[l] = (d_.ib_off[l] + ((N + 15) & ~15)) / 4;
                pp_.ldw4[l] = fl_ldw(K) / 4;
                pp_.k4[l] = ((K + 15) & ~15) / 4;
                pp_.pk_w[l] = e_.w_off[l] - e_.param_off;
                pp_.pk_lda[l] = e_.ldw[l];
                pp_.pk_b[l] = e_.bias_off[l] - e_.param_off;
            }
        }
    }
    bool has_peer() const { return peer_ != nullptr; }

    // Enable (ptr != 0) / disable in-kernel phase stamps: [blocks, 16] uint64 buffer.
    // (a configuration change like any other: cached graphs hold the old stamp buffer)
    void set_debug(uintptr_t ptr) {
        b_.dbg = as_ptr<unsigned long long>(ptr);
        drop_graph();
    }

    // Held-out scoring (fl_heldout.hip): every round the engine aggregates then ends with the row and
    // fold launches on its output image; `X` = 0 turns it off.  All buffers are caller-owned device
    // memory (fl_common.h FLHeldout).  Kernel arguments and the round kind change (no lagged rounds
    // while it is on), so captured graphs are dropped, as by set_debug.
    void set_heldout(uintptr_t X, uintptr_t y, int n, uintptr_t scratch, uintptr_t hist_cm, uintptr_t hist_loss,
                     uintptr_t best_image, uintptr_t best, bool keep_best) {
        FLHeldout h;
        std::memset(&h, 0, sizeof(h));
        if (X != 0) {
            if (n < 1 || n > FL_HELDOUT_MAX_ROWS)
                throw std::runtime_error("set_heldout: 1 .. 2^24 held-out rows, got " + std::to_string(n));
            if (!y || !scratch || !hist_cm || !hist_loss || (keep_best && (!best_image || !best)))
                throw std::runtime_error("set_heldout: missing buffers");
            h.X = as_ptr<const float>(X);
            h.y = as_ptr<const int>(y);
            h.n = n;
            h.max_rounds = c_.max_rounds;
            h.keep_best = keep_best ? 1 : 0;
            h.scratch = as_ptr<int>(scratch);
            h.hist_cm = as_ptr<int>(hist_cm);
            h.hist_loss = as_ptr<float>(hist_loss);
            h.best_image = keep_best ? as_ptr<float>(best_image) : nullptr;
            h.best = keep_best ? as_ptr<float>(best) : nullptr;
            prepare_heldout();
        }
        ho_ = h;
        tr_.heldout_on = X != 0;
        refresh_undo();
        drop_graph();
    }
    bool heldout() const { return tr_.heldout_on; }
    int heldout_rows_per_block() const { return ho_R(); }

    // Row mode of the held-out kernel: softmax probabilities [n][C] and / or the logits' first-maximum
    // argmax [n] of the fp32 image `params` on rows [0, n) of X (either output may be 0).
    void predict(uintptr_t X, int n, uintptr_t params, uintptr_t proba, uintptr_t pred, uintptr_t stream) {
        prepare_heldout();
        HIP_CHECK(fl_launch_heldout_predict(dh_, ho_R(), as_ptr<const float>(X), n, as_ptr<const float>(params),
                                            as_ptr<float>(proba), as_ptr<int>(pred), as_stream(stream)));
    }

    // Launch one kernel of round r on its live state (0 = train, 1 = adam, 2 = eval).
    void launch_one(int r, int which, uintptr_t stream) {
        issue([&](RoundPlan& p) { plan_relaunch(p, "launch_one", r, which); }, as_stream(stream), nullptr);
    }

    // Per-kernel device time (us, averaged over `iters` back-to-back launches, hipEvents)
    // re-running the kernels of the last issued round `r` on its (live) state.  Training
    // launches use local_step=1 semantics so the round state is not advanced.
    py::dict time_kernels(int r, int iters, uintptr_t stream) {
        hipStream_t s = as_stream(stream);
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        py::dict out;
        auto timeit = [&](const char* name, int which) {
            // (planned per launch: the first train launch consumes a pending repack)
            auto launch = [&] { issue([&](RoundPlan& p) { plan_relaunch(p, "time_kernels", r, which); }, s, nullptr); };
            launch();
            HIP_CHECK(hipEventRecord(e0, s));
            for (int i = 0; i < iters; ++i) launch();
            HIP_CHECK(hipEventRecord(e1, s));
            HIP_CHECK(hipEventSynchronize(e1));
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            out[name] = 1e3 * ms / iters;
        };
        timeit("train", 0);
        timeit("adam", 1);
        timeit("eval", 2);
        HIP_CHECK(hipEventDestroy(e0));
        HIP_CHECK(hipEventDestroy(e1));
        return out;
    }

    // Per-kernel device time of the REAL round design (us per round, by kernel kind): rounds
    // [r0, r0 + n) are issued eagerly exactly as run() issues them, with a hipEvent after every
    // launch; a sleeping gate kernel holds the stream until the whole sequence is enqueued, so
    // the kernels run back to back (host launch pace does not leak into the intervals).  The
    // interval before a kernel's event is charged to that kernel: launch gaps on the device
    // are included (that is what a graph replay pays too, minus the graph's own launch cost).
    // With the Adam-fused peer exchange, waiting for slower ranks shows up under "adam".
    // `warm` untraced rounds run first behind the gate (they absorb the ranks' start skew: the
    // first in-kernel exchange waits for the last rank to arrive).
    py::dict trace(int r0, int n, uintptr_t stream, RcclComm* comm, bool close, double gate_us, int warm) {
        if (n < 1 || warm < 0) throw std::runtime_error("trace: n >= 1, warm >= 0");
        hipStream_t s = as_stream(stream);
        std::vector<std::pair<int, hipEvent_t>> ev;
        hipEvent_t e0;
        HIP_CHECK(hipEventCreateWithFlags(&e0, trace_event_flags()));
        HIP_CHECK(fl_launch_gate(gate_us, s));
        if (warm > 0) run(r0, warm, stream, comm, false);
        HIP_CHECK(hipEventRecord(e0, s));
        tev_ = &ev;
        try {
            run(r0 + warm, n, stream, comm, close);
        } catch (...) {
            tev_ = nullptr;
            throw;
        }
        tev_ = nullptr;
        HIP_CHECK(hipStreamSynchronize(s));
        constexpr int TR_N = FLLaunchRec::N_KINDS;  // events are tagged with the launch kind
        static const char* names[TR_N] = {"pack", "train", "adam", "eval", "allreduce", "eval_fedavg", "dp",
                                          "server", "finalize", "compress", "heldout"};
        double us[TR_N] = {0};
        int cnt[TR_N] = {0};
        hipEvent_t prev = e0;
        for (auto& [what, e] : ev) {
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, prev, e));
            us[what] += 1e3 * ms;
            ++cnt[what];
            prev = e;
        }
        float total = 0.f;
        HIP_CHECK(hipEventElapsedTime(&total, e0, prev));
        py::dict out, launches;
        for (int k = 0; k < TR_N; ++k)
            if (cnt[k]) {
                out[names[k]] = us[k] / n;
                launches[names[k]] = cnt[k];
            }
        out["round"] = 1e3 * total / n;
        out["launches"] = launches;
        out["rounds"] = n;
        for (auto& pe : ev) hipEventDestroy(pe.second);
        hipEventDestroy(e0);
        return out;
    }

    // held-out evaluation: confusion matrix of `params` on (X, y) accumulated into cm_out
    void confusion(uintptr_t X, uintptr_t y, int n_rows, uintptr_t params, uintptr_t cm_out, uintptr_t stream) {
        HIP_CHECK(fl_launch_confusion(d_, c_.R, as_ptr<const float>(X), as_ptr<const int>(y), n_rows,
                                      as_ptr<const float>(params), as_ptr<float>(cm_out), as_stream(stream)));
    }

    py::dict layout() const {
        py::dict o;
        std::vector<int> w, bb, iw, ib, ld, dims;
        for (int l = 0; l < d_.L; ++l) {
            w.push_back(d_.w_off[l]); bb.push_back(d_.b_off[l]);
            iw.push_back(d_.iw_off[l]); ib.push_back(d_.ib_off[l]);
        }
        for (int l = 0; l <= d_.L; ++l) { ld.push_back(d_.ld[l]); dims.push_back(d_.dim[l]); }
        o["P"] = d_.P;
        o["Pimg"] = d_.Pimg;
        o["w_off"] = w;
        o["b_off"] = bb;
        o["iw_off"] = iw;
        o["ib_off"] = ib;
        o["ld"] = ld;
        o["dims"] = dims;
        o["lds_bytes"] = dtype_ == 0 ? d_.lds_floats * 4 : e_.lds_bytes;
        o["bank_level"] = dtype_ == 0 ? -1 : e_.level;
        o["eval_lds_bytes"] = dtype_ == 0 ? d_.lds_floats * 4 : ev_.lds_bytes;
        // bf16: the packed image (packed_global / packed_local) is [W hi | fp32 biases | W lo], each
        // lo element wlo_delta bytes behind its hi element; param_bytes in all
        o["wlo_delta"] = dtype_ == 1 ? e_.wlo_delta : 0;
        o["param_bytes"] = dtype_ == 1 ? e_.param_bytes : 0;
        o["lag_reg"] = dtype_ == 1 && e_.lag_reg != 0;  // lagged rounds score in registers (fl_layout.h)
        o["plain_fwd"] = c_.plain_fwd != 0;              // plain-bf16 training forward (several clients)
        o["split_score"] = c_.split_score != 0;          // lagged scoring on workgroups of its own
        // the train kernel of classic / fused rounds is the reference shape's specialised one
        o["shape_spec"] = shape_spec_on_ && (dtype_ == 1 ? fl_train_bf16_spec_ok(d_, e_, c_, FL_EVAL_FUSED)
                                                         : fl_train_spec_ok(d_, c_, FL_EVAL_FUSED));
        o["adam_spec"] = adam_spec_ok();  // the Adam kernel of those rounds is the specialised one
        o["eval_fedavg"] = peer_ != nullptr && !tr_.fused && tr_.eval_fedavg_fits;
        // the peer call selects / opens instead of summing (peer_select.h): "none", "robust", "secagg"
        o["peer_select"] = std::string(peer_ == nullptr || sel_.mode == 0 ? "none"
                                       : sel_.mode == PEER_SELECT_ROBUST ? "robust" : "secagg");
        o["dtype"] = dtype_;
        o["slab_stride"] = c_.slab_stride;
        o["n_slabs"] = c_.n_slabs;
        o["slab_f16"] = c_.slab_f16;
        // the slab rows are blocked rows (fl_layout.h FlSlabBlk; slab_map() gives each dense index's position)
        o["slab_blocked"] = slab_blocked_;
        // the specialised bf16 train kernel runs its exchanged epilogues (fl_layout.h fl_epi_*)
        o["epi_exchange"] = epi_exchange_;
        o["tail_off"] = c_.tail_off;
        o["tail_stride"] = c_.tail_stride;
        o["tail_len"] = c_.tail_len;
        o["comm_len"] = comm_len_;
        o["lagged_eval"] = lagged();
        o["dp"] = tr_.dp_on;                               // clipped (+ noised) contributions, classic rounds
        {
            // compression of every contribution (a simulated uplink: the exchange stays dense), classic rounds
            static const char* compress_names[] = {"none", "topk", "sign", "qsgd", "randk"};
            const long long P = d_.P, k = tr_.compress_on ? cp_.k : P;
            long long code_bits = 0;  // qsgd: ceil(log2(2 s + 1)), a fixed-width sign-and-level code
            while ((1ll << code_bits) < 2ll * cp_.levels + 1) ++code_bits;
            py::dict c;
            c["kind"] = std::string(compress_names[cp_.kind]);
            c["k"] = (int)k;
            c["dense_bytes"] = 4 * P;
            c["uplink_bytes"] = cp_.kind == FL_COMPRESS_TOPK   ? 8 * k
                                : cp_.kind == FL_COMPRESS_SIGN ? 4 + (P + 7) / 8
                                : cp_.kind == FL_COMPRESS_QSGD ? 4 + (P * code_bits + 7) / 8
                                : cp_.kind == FL_COMPRESS_RANDK ? 4 * k
                                                               : 4 * P;
            if (cp_.kind == FL_COMPRESS_QSGD) c["levels"] = cp_.levels;
            o["compress"] = c;
        }
        static const char* server_names[] = {"none", "sgd", "adagrad", "adam", "yogi"};
        o["server_opt"] = std::string(server_names[sv_.kind]);  // server step after every aggregation, classic rounds
        o["state_bytes"] = (int)sizeof(FLState);
        return o;
    }

    // Position (in slab elements from the row's start) of every dense parameter index: the identity for
    // dense rows, fl_slab_blk_pos for blocked ones (layout()["slab_blocked"]).
    std::vector<int> slab_map() const {
        std::vector<int> pos((size_t)d_.P);
        const FlSlabBlk sb = FlRefSlabBlk<32>::s;
        for (int di = 0; di < d_.P; ++di) pos[(size_t)di] = slab_blocked_ ? fl_slab_blk_pos(d_, sb, di) : di;
        return pos;
    }

  private:
    // Plan with `plan`, then execute the records in order.  A planning error leaves the carry as
    // it was and nothing issued.
    template <class F>
    void issue(F&& plan, hipStream_t s, RcclComm* comm) {
        RoundPlan p;
        const RoundCarry carry0 = carry_;
        try {
            plan(p);
        } catch (...) {
            carry_ = carry0;
            throw;
        }
        for (const FLLaunchRec& m : p) execute(m, s, comm);
    }
    void issue_round(int r, hipStream_t s, RcclComm* comm, bool lag) {
        issue([&](RoundPlan& p) { plan_round(tr_, carry_, p, r, true, lag, true, comm != nullptr); }, s, comm);
    }
    // Records that re-run one kernel of round r on its live state (0 = train, 1 = Adam, both as a
    // later local step; 2 = eval; 3 = bf16: the lagged first train step, which advances the state).
    // Not where the round's output is not the aggregated local model: the Adam kernel alone would
    // republish w * local over the noised contribution / the server step's image.
    void plan_relaunch(RoundPlan& p, const char* what, int r, int which) {
        if (tr_.dp_on) throw std::runtime_error(std::string(what) + ": not on a DP engine (use trace)");
        if (tr_.compress_on) throw std::runtime_error(std::string(what) + ": not on a compressing engine (use trace)");
        if (tr_.server_on)
            throw std::runtime_error(std::string(what) + ": not on a server-optimizer engine (use trace)");
        const int par = (r + 1) & 1;
        const FLSel pg = fl_at(FL_TB_PBUF0 + (r & 1)), so = fl_at(FL_TB_ST0 + par);
        if (which == 0) plan_train_launch(tr_, carry_, p, par, pg, so, so, 1);
        else if (which == 1)
            p.push(FLLaunchRec::ADAM, 1, 0, 0, FL_FOLD_B, par, fl_at(FL_TB_LOCAL), pg, plan_comm_buf(tr_, par), so);
        else if (which == 3 && dtype_ == 1 && slab_blocked_)
            throw std::runtime_error(std::string(what) + ": no lagged train step on an engine with the blocked slab row");
        else if (which == 3 && dtype_ == 1)
            plan_train_launch(tr_, carry_, p, par, pg, so, so, 0, FL_EVAL_LAGGED, fl_at(FL_TB_LAG), 0);
        else plan_eval(tr_, p, r);
    }

    // FL_TB_* slot -> pointer: the trial table's eight bases, then the peer's two send buffers
    void fill_bases() {
        char* const bases[FL_TB_COMM1 + 1] = {
            (char*)pbuf_[0], (char*)pbuf_[1], (char*)st_[0], (char*)st_[1], (char*)b_.local, (char*)lagbuf_,
            b_.pk_global, b_.pk_local, peer_ != nullptr ? (char*)peer_->send(0) : nullptr,
            peer_ != nullptr ? (char*)peer_->send(1) : nullptr};
        std::memcpy(base_, bases, sizeof(base_));
    }
    // Issue one planned launch on `s` (`comm`: the RCCL communicator of an ALLREDUCE without a peer).
    void execute(const FLLaunchRec& m, hipStream_t s, RcclComm* comm = nullptr) {
        auto F = [&](int k) { return m.p[k].base < 0 ? nullptr : (float*)(base_[m.p[k].base] + m.p[k].off); };
        auto S = [&](int k) { return (FLState*)F(k); };
        const MLPDescB* eb = dtype_ == 1 ? &e_ : nullptr;
        const int* i = m.i;
        switch (m.kind) {
            case FLLaunchRec::PACK:
                HIP_CHECK(fl_launch_pack_bf16(d_, e_, F(0), (char*)F(1), s));
                break;
            case FLLaunchRec::TRAIN:
                if (dtype_ == 0) HIP_CHECK(fl_launch_train(d_, c_, b_, F(0), S(1), S(2), i[0], s, i[2], F(3), i[3],
                                                              shape_spec_on_));
                else
                    HIP_CHECK(fl_launch_train_bf16(d_, e_, c_, b_, F(0), S(1), S(2), i[0], s, i[1] != 0, i[2], F(3),
                                                   i[3], shape_spec_on_, slab_blocked_, epi_exchange_));
                break;
            case FLLaunchRec::ADAM: {
                PeerArgs pa;
                if (m.peer) pa = peer_->args(m.par, pbuf_[m.par]);
                HIP_CHECK(fl_launch_adam(d_, c_, b_, F(0), F(1), F(2), S(3), i[0], s, eb, S(4), i[1], i[2], i[3],
                                         m.peer ? &pa : nullptr, (m.peer >> 1) & 1, (m.peer >> 2) & 1, adam_spec_allowed(),
                                         slab_blocked_));
                break;
            }
            case FLLaunchRec::EVAL:
                ++eval_launches_;
                if (dtype_ == 0) HIP_CHECK(fl_launch_eval(d_, c_, b_, F(0), F(1), S(2), s));
                else HIP_CHECK(fl_launch_eval_bf16(d_, ev_, c_, b_, F(0), F(1), S(2), s));
                break;
            case FLLaunchRec::ALLREDUCE:
                if (sel_.mode != 0) {
                    // robust rule / secure aggregation: select or open over the peers' send buffers under the
                    // round's state (that of the output parity); never a sum
                    if (peer_ == nullptr)
                        throw std::runtime_error("FLEngine: a robust rule / secure aggregation aggregates over the "
                                                 "peer plane or from the caller, not over RCCL");
                    if (sel_.mode == PEER_SELECT_OPEN)  // this rank's contribution becomes its masked words, in place
                        HIP_CHECK(fl_launch_secagg_mask(d_, sel_.sa, (float* const*)sa_tab_ + m.par, 1,
                                                        (uint32_t* const*)sa_tab_ + 2, st_[m.par], s));
                    HIP_CHECK(peer_->launch_select(m.par, pbuf_[m.par], dtype_ == 1 ? &pp_ : nullptr, sel_, st_[m.par], s));
                } else if (peer_ != nullptr) {
                    HIP_CHECK(peer_->launch(m.par, pbuf_[m.par], dtype_ == 1 ? &pp_ : nullptr, s));
                } else {
                    comm->allreduce_f32((uintptr_t)pbuf_[m.par], (size_t)comm_len_, (uintptr_t)s);
                }
                break;
            case FLLaunchRec::EVAL_FEDAVG: {
                const PeerArgs a = peer_->args(m.par, pbuf_[m.par], d_.Pimg);
                PeerPack pk;
                std::memset(&pk, 0, sizeof(pk));
                if (dtype_ == 1) pk = pp_;
                if (dtype_ == 0) HIP_CHECK(fl_launch_eval_fedavg(d_, c_, b_, F(0), F(1), S(2), a, pk, s));
                else HIP_CHECK(fl_launch_eval_fedavg_bf16(d_, ev_, c_, b_, F(0), F(1), S(2), a, pk, s));
                break;
            }
            case FLLaunchRec::DP:
                HIP_CHECK(fl_launch_dp(d_, dp_, F(0), F(1), F(2), S(3), b_.rtab, s));
                break;
            case FLLaunchRec::COMPRESS:
                HIP_CHECK(fl_launch_compress(d_, cp_, F(0), F(1), F(2), S(3), b_.rtab, s));
                break;
            case FLLaunchRec::SERVER:
                HIP_CHECK(fl_launch_server(d_, sv_, F(0), F(1), S(2), eb, dtype_ == 1 ? b_.pk_global : nullptr, s));
                break;
            case FLLaunchRec::HELDOUT:  // the row launch, then the fold launch
                HIP_CHECK(fl_launch_heldout(dh_, ho_R(), ho_, F(0), S(1), s));
                break;
            case FLLaunchRec::FINALIZE:
                HIP_CHECK(fl_launch_finalize(d_, c_, b_, F(0), S(1), S(2), s, i[0],
                                             late_fold() ? pbuf_[m.par] : nullptr));
                break;
            default: throw std::runtime_error("FLEngine: unknown launch");
        }
        mark(m.kind, s);
    }

    struct GraphRec {
        int n;                 // rounds
        hipGraph_t g;
        hipGraphExec_t e;
        long long evals;       // evaluation kernels per replay
        RcclComm* comm;        // communicator the rounds were captured with
    };
    static constexpr int kMaxGraphs = 4;
    static void destroy_rec(GraphRec& r) {
        if (r.e) hipGraphExecDestroy(r.e);
        if (r.g) hipGraphDestroy(r.g);
        r.e = nullptr;
        r.g = nullptr;
    }
    void select_graph(int i) {
        graph_ = graphs_[i].g;
        exec_ = graphs_[i].e;
        graph_rounds_ = graphs_[i].n;
        graph_evals_ = graphs_[i].evals;
    }
    void drop_graph() {
        for (auto& r : graphs_) destroy_rec(r);
        graphs_.clear();
        exec_ = nullptr;
        graph_ = nullptr;
        graph_rounds_ = 0;
    }
    std::vector<GraphRec> graphs_;
    long long captures_ = 0;   // graphs captured + instantiated (not counting cache hits)

    MLPDesc d_;
    MLPDescB e_;
    MLPDescB ev_;  // evaluation-only layout of e_ (no delta buffers)
    int dtype_ = 0;  // 0 = fp32 MFMA, 1 = bf16 MFMA (fp32 accumulate / master weights)
    bool shape_spec_on_ = true;  // FEDMI_SHAPE_SPEC != 0: launchers may pick shape-specialised kernels
    bool adam_spec_on_ = true;   // ... and FEDMI_ADAM_SPEC != 0: the Adam launcher too
    bool slab_blocked_ = false;  // the fp16 slab rows are blocked rows (fl_layout.h FlSlabBlk; see the constructor)
    bool epi_exchange_ = false;  // the specialised bf16 train kernel's exchanged epilogues (see the constructor)
    // The engine allows the specialised Adam kernel: no peer plane, and the round's output is the
    // Adam kernel's own (no DP clip, no compression, no server step after it); the launcher checks the shape, the
    // client count, the lag region and the undo buffer per launch (fl_adam_spec_ok).
    bool adam_spec_allowed() const { return adam_spec_on_ && peer_ == nullptr && !tr_.foreign_output(); }
    bool adam_spec_ok() const {
        return adam_spec_allowed() && fl_adam_spec_ok(d_, dtype_ == 1 ? &e_ : nullptr, c_, b_);
    }
    char* pk_ = nullptr;
    float* lagbuf_ = nullptr;  // FL_EVAL_LAGGED count + loss carry-over
    long long comm_len_ = 0;   // floats of a comm buffer: image + tails (+ lag region)
    RoundTraits tr_;           // round kind: fixed after construction / attach_peer
    RoundCarry carry_;         // what the last issued round left pending
    PeerAllReduce* peer_ = nullptr;  // one-shot xGMI all-reduce (nullptr: RCCL)
    float* undo_ = nullptr;          // FLBuffers::undo storage (lagged engines with early stopping)
    PeerPack pp_;                    // its bf16 pack epilogue (bf16 mode)
    PeerSelect sel_;                 // mode != 0: the peer call selects (robust rule) or opens (secure aggregation)
    uint32_t* sa_clamp_ = nullptr;   // secure aggregation: this client's clamp history [max_rounds] (caller-owned)
    void** sa_tab_ = nullptr;        // ... device pointer tables of the mask launch: {send 0, send 1, clamp history}
    FLDp dp_;                  // differential privacy: fl_dp_kernel after every round's last Adam kernel
    FLCompress cp_;            // compression: fl_compress_kernel after every round's last Adam kernel
    bool compress_random() const { return cp_.kind == FL_COMPRESS_QSGD || cp_.kind == FL_COMPRESS_RANDK; }
    FLServer sv_;              // server optimizer: fl_server_kernel after every round's aggregation
    FLHeldout ho_ = {};        // held-out scoring: fl_heldout row + fold launches at the end of every round
    MLPDesc dh_ = {};          // ... the fp32 forward layout at its rows per workgroup (prepare_heldout)
    // rows per workgroup of the held-out kernels: the engine's, at most 32 (the fp32 forward's tiles)
    int ho_R() const { return c_.R > 32 ? 32 : c_.R; }
    void prepare_heldout() {
        if (dh_.L != 0) return;
        MLPDesc d;
        fl_build_fp32_layout(d_.dim, d_.L, ho_R(), &d);
        if ((size_t)d.lds_floats * 4 > FL_LDS_DYNAMIC_MAX)
            throw std::runtime_error("FLEngine: the fp32 forward pass of the held-out kernels exceeds LDS");
        HIP_CHECK(fl_set_lds_limit_heldout((size_t)d.lds_floats * 4));
        dh_ = d;
    }
    FLConfig c_;
    FLBuffers b_;
    float* pbuf_[2];
    FLState* st_[2];
    char* base_[FL_TB_COMM1 + 1];  // FL_TB_* slot -> pointer (fill_bases)
    hipGraph_t graph_ = nullptr;
    hipGraphExec_t exec_ = nullptr;
    int graph_rounds_ = 0;
    long long eval_launches_ = 0;  // see eval_launches()
    long long graph_evals_ = 0;    // evaluation kernels inside the captured graph
    // trace(): an event after every launch, tagged with the launch kind
    std::vector<std::pair<int, hipEvent_t>>* tev_ = nullptr;
    // trace markers without the system-scope release/acquire (device-side timing only needs the
    // marker's timestamp); FEDMI_TRACE_SYSFENCE=1 restores default events (A/B)
    static unsigned trace_event_flags() {
        const char* v = std::getenv("FEDMI_TRACE_SYSFENCE");
        return (v != nullptr && v[0] == '1') ? hipEventDefault : hipEventDisableSystemFence;
    }
    void mark(int what, hipStream_t s) {
        if (tev_ == nullptr) return;
        hipEvent_t e;
        HIP_CHECK(hipEventCreateWithFlags(&e, trace_event_flags()));
        tev_->emplace_back(what, e);
        HIP_CHECK(hipEventRecord(e, s));
    }
};

// ---------------------------------------------------------------------------------------
// Trial batch (fl_common.h FLTrialDesc): K engines of one shape run every kernel of a round as
// ONE launch with a trial grid dimension.  Each engine's round logic (state machine, modes,
// buffer parities) runs unchanged in recording mode; the recorded launches of the K engines
// are matched launch by launch and issued batched.  Engines are ordered by local steps,
// descending, so the trials taking part in a later local step are a prefix of the table.
// ---------------------------------------------------------------------------------------
class TrialBatch {
  public:
    explicit TrialBatch(std::vector<FLEngine*> engs) : engs_(std::move(engs)) {
        K_ = (int)engs_.size();
        if (K_ < 1) throw std::runtime_error("TrialBatch: no engines");
        const FLEngine& a = *engs_[0];
        for (int k = 0; k < K_; ++k) {
            const FLEngine& e = *engs_[k];
            if (e.peer_ != nullptr) throw std::runtime_error("TrialBatch: engines must not use the peer all-reduce");
            if (e.tr_.server_on) throw std::runtime_error("TrialBatch: no server optimizer (server_opt)");
            if (e.tr_.compress_on) throw std::runtime_error("TrialBatch: no compression (compress)");
            if (e.tr_.heldout_on) throw std::runtime_error("TrialBatch: no held-out scoring (set_heldout)");
            // the batch kernels write and read dense slab rows: from here on the engine's own launches do
            // too (the row stride stays; train / Adam pairs are issued together, so no pair is split)
            engs_[k]->slab_blocked_ = false;
            if (e.dtype_ != a.dtype_ || std::memcmp(&e.d_, &a.d_, sizeof(MLPDesc)) != 0 ||
                (a.dtype_ == 1 && (std::memcmp(&e.e_, &a.e_, sizeof(MLPDescB)) != 0 ||
                                   std::memcmp(&e.ev_, &a.ev_, sizeof(MLPDescB)) != 0)))
                throw std::runtime_error("TrialBatch: engines differ in shape or dtype");
            if (e.c_.R != a.c_.R || e.c_.n_rows != a.c_.n_rows || e.c_.world != a.c_.world ||
                e.c_.plain_fwd != a.c_.plain_fwd ||
                e.c_.rank != a.c_.rank || e.c_.slab_f16 != a.c_.slab_f16 || e.c_.lag_off != a.c_.lag_off ||
                e.tr_.fused != a.tr_.fused || e.lagged() != a.lagged() || e.tr_.emulate != a.tr_.emulate)
                throw std::runtime_error("TrialBatch: engines differ in rows, clients or round kind");
            if (k > 0 && e.c_.local_steps > engs_[k - 1]->c_.local_steps)
                throw std::runtime_error("TrialBatch: order the engines by local steps, descending");
        }
        HIP_CHECK(hipMalloc(&dT_, sizeof(FLTrialDesc) * K_));
        plans_.resize(K_);
        carry0_.resize(K_);
        upload(nullptr);
    }
    ~TrialBatch() {
        if (dT_) (void)hipFree(dT_);
    }
    int size() const { return K_; }

    // Rounds [r0, r0 + n) of every trial (FLEngine::run without a communicator).
    void run(int r0, int n, uintptr_t stream, bool close) {
        for (int r = r0; r < r0 + n; ++r) {
            const bool last = close && r == r0 + n - 1;
            issue([&](FLEngine& e, RoundPlan& p) {
                plan_round(e.tr_, e.carry_, p, r, true, e.lagged() && !last, true, false);
            }, as_stream(stream));
        }
    }
    // Local part of round r of every trial (the caller reduces the trials' shared buffer).
    void run_local(int r, uintptr_t stream) {
        issue([&](FLEngine& e, RoundPlan& p) { plan_round(e.tr_, e.carry_, p, r, false, false, false, false); },
              as_stream(stream));
    }
    void finalize(int r, uintptr_t stream) {
        issue([&](FLEngine& e, RoundPlan& p) { plan_finalize(e.tr_, e.carry_, p, r); }, as_stream(stream));
    }
    bool needs_eager_round() const {
        for (auto* e : engs_)
            if (e->needs_eager_round()) return true;
        return false;
    }

  private:
    void build_table(std::vector<FLTrialDesc>& T) const {
        T.assign(K_, FLTrialDesc{});
        for (int k = 0; k < K_; ++k) {
            const FLEngine& e = *engs_[k];
            T[k].c = e.c_;
            T[k].b = e.b_;
            std::memcpy(T[k].base, e.base_, sizeof(T[k].base));
        }
    }
    // (re)upload the table when an engine's configuration changed (e.g. set_early_stop);
    // never inside a stream capture
    void upload(hipStream_t s) {
        std::vector<FLTrialDesc> T;
        build_table(T);
        if (!host_.empty() && std::memcmp(T.data(), host_.data(), sizeof(FLTrialDesc) * K_) == 0) return;
        if (s != nullptr) {
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            HIP_CHECK(hipStreamIsCapturing(s, &cs));
            if (cs != hipStreamCaptureStatusNone)
                throw std::runtime_error("TrialBatch: a trial's configuration changed during a graph capture");
            HIP_CHECK(hipStreamSynchronize(s));  // kernels still reading the old table
        }
        HIP_CHECK(hipMemcpy(dT_, T.data(), sizeof(FLTrialDesc) * K_, hipMemcpyHostToDevice));
        host_ = std::move(T);
    }
    // What a batched launch cannot do (the constructor already refuses peer and server engines).
    static void check_batchable(const FLLaunchRec& m) {
        if (m.kind == FLLaunchRec::DP) throw std::runtime_error("trial batch: no DP");
        if (m.kind == FLLaunchRec::COMPRESS) throw std::runtime_error("trial batch: no compression");
        if (m.kind == FLLaunchRec::SERVER) throw std::runtime_error("trial batch: no server optimizer");
        if (m.kind == FLLaunchRec::HELDOUT) throw std::runtime_error("trial batch: no held-out scoring");
        if (m.kind == FLLaunchRec::ALLREDUCE || m.kind == FLLaunchRec::EVAL_FEDAVG)
            throw std::runtime_error("trial batch: no peer all-reduce");
        if (m.kind == FLLaunchRec::ADAM && m.peer) throw std::runtime_error("trial batch: no in-kernel exchange");
    }

    // Plan every engine's launches and match them into batched launches (all checks done before
    // anything is issued: on a mismatch the engines' carries are rolled back and nothing ran),
    // then issue them.  cnt_[j]: trials taking part in engine 0's j-th launch, a prefix of the table.
    template <class F>
    void issue(F&& plan_one, hipStream_t s) {
        upload(s);
        for (int k = 0; k < K_; ++k) carry0_[k] = engs_[k]->carry_;
        const RoundPlan& lead = plans_[0];
        try {
            for (int k = 0; k < K_; ++k) {
                plans_[k].n = 0;
                plan_one(*engs_[k], plans_[k]);
                for (const FLLaunchRec& m : plans_[k]) {
                    check_batchable(m);
                    if (m.kind == FLLaunchRec::EVAL) ++engs_[k]->eval_launches_;
                }
            }
            std::vector<int> pos(K_, 0);
            for (int j = 0; j < lead.n; ++j) {
                int cnt = 0;
                for (int k = 0; k < K_; ++k) {
                    const bool match = pos[k] < plans_[k].n && same_launch(plans_[k].rec[pos[k]], lead.rec[j]);
                    if (match && k != cnt) throw std::runtime_error("TrialBatch: launch sequences do not align");
                    if (match && !same_buffers(plans_[k].rec[pos[k]], lead.rec[j]))
                        throw std::runtime_error("TrialBatch: trials disagree on a launch argument");
                    if (match) ++cnt;
                }
                for (int k = 0; k < cnt; ++k) ++pos[k];
                cnt_[j] = cnt;
            }
            for (int k = 0; k < K_; ++k)
                if (pos[k] != plans_[k].n) throw std::runtime_error("TrialBatch: launch sequences do not align");
        } catch (...) {
            for (int k = 0; k < K_; ++k) engs_[k]->carry_ = carry0_[k];
            throw;
        }
        for (int j = 0; j < lead.n; ++j) launch(*engs_[0], lead.rec[j], lead.rec[j].p, cnt_[j], s);
    }
    void launch(const FLEngine& e, const FLLaunchRec& m, const FLSel* sel, int cnt, hipStream_t s) {
        const FLConfig& c = e.c_;
        switch (m.kind) {
            case FLLaunchRec::PACK:
                HIP_CHECK(fl_launch_pack_bf16_batch(e.d_, e.e_, dT_, cnt, sel[0], sel[1], s));
                break;
            case FLLaunchRec::TRAIN:
                if (e.dtype_ == 0)
                    HIP_CHECK(fl_launch_train_batch(e.d_, c.R, c.n_slabs, dT_, cnt, sel[0], sel[1], sel[2], m.i[0],
                                                    m.i[2], sel[3], m.i[3], s));
                else
                    HIP_CHECK(fl_launch_train_bf16_batch(e.d_, e.e_, c.R, c.n_slabs, dT_, cnt, sel[0], sel[1], sel[2],
                                                         m.i[0], m.i[1], m.i[2], sel[3], m.i[3], s, c.plain_fwd));
                break;
            case FLLaunchRec::ADAM:
                HIP_CHECK(fl_launch_adam_batch(e.d_, e.dtype_ == 1 ? &e.e_ : nullptr, dT_, cnt, sel[0], sel[1], sel[2],
                                               sel[3], m.i[0], sel[4], m.i[1], m.i[2], m.i[3], s));
                break;
            case FLLaunchRec::EVAL:
                if (e.dtype_ == 0)
                    HIP_CHECK(fl_launch_eval_batch(e.d_, c.R, c.n_rows, dT_, cnt, sel[0], sel[1], sel[2], s));
                else
                    HIP_CHECK(fl_launch_eval_bf16_batch(e.d_, e.ev_, c.R, c.n_rows, dT_, cnt, sel[0], sel[1], sel[2],
                                                        s));
                break;
            case FLLaunchRec::FINALIZE:
                HIP_CHECK(fl_launch_finalize_batch(e.d_, dT_, cnt, sel[0], sel[1], sel[2], m.i[0], s));
                break;
            default: throw std::runtime_error("TrialBatch: unknown launch");
        }
    }

    std::vector<FLEngine*> engs_;
    int K_ = 0;
    FLTrialDesc* dT_ = nullptr;
    std::vector<FLTrialDesc> host_;
    std::vector<RoundPlan> plans_;    // per engine, reused by every issue()
    std::vector<RoundCarry> carry0_;  // the engines' carries before planning (rollback)
    int cnt_[FL_PLAN_CAP];
};

// Thin wrappers used by tests and the synthetic-data path.
static void synth(uintptr_t X, uintptr_t y, long long n, int F, unsigned long long seed, unsigned long long off,
                  uintptr_t w1, uintptr_t w2, int H, uintptr_t stream, float label_noise) {
    HIP_CHECK(fl_launch_synth(as_ptr<float>(X), as_ptr<int>(y), n, F, seed, off, as_ptr<const float>(w1),
                              as_ptr<const float>(w2), H, as_stream(stream), label_noise));
}

// Image descriptor of `dims` for the stand-alone launches below (`who` names the caller in the refusal).
static MLPDesc desc_of(const std::vector<int>& dims, const char* who) {
    const int L = (int)dims.size() - 1;
    if (L < 1 || L > FL_MAX_LAYERS) throw std::runtime_error(std::string(who) + ": 1..4 Linear layers supported");
    MLPDesc d;
    fl_build_fp32_layout(dims.data(), L, 16, &d);
    return d;
}

// Robust aggregate (fl_robust.hip) over K buffers of the image of `dims` + `tails_len` floats.  `src` /
// `dst`: device tables of K / n_dst buffer addresses (int64); `state` / `rtab`: a client's round
// state and per-round table.  Works across engines' buffers, so it is not an FLEngine phase.
static void robust_aggregate(std::vector<int> dims, int kind, double beta, uintptr_t src, int K, uintptr_t dst,
                             int n_dst, uintptr_t state, uintptr_t rtab, int tails_len, int max_rounds,
                             uintptr_t stream, uintptr_t keep) {
    const MLPDesc d = desc_of(dims, "robust_aggregate");
    if (K < 1 || K > FL_ROBUST_MAX_K)
        throw std::runtime_error("robust_aggregate: 1.." + std::to_string(FL_ROBUST_MAX_K) +
                                 " clients (the width of the sampled-client mask), got " + std::to_string(K));
    if (kind != FL_ROBUST_MEDIAN && kind != FL_ROBUST_TRIMMED)
        throw std::runtime_error("robust_aggregate: kind must be 1 (median) or 2 (trimmed mean)");
    if (!(beta >= 0.0 && beta < 0.5)) throw std::runtime_error("robust_aggregate: beta must be in [0, 0.5)");
    if (n_dst < 1 || n_dst > FL_ROBUST_MAX_K || tails_len < 0 || max_rounds < 1 || !src || !dst || !state || !rtab)
        throw std::runtime_error("robust_aggregate: bad arguments");
    FLRobust p;
    std::memset(&p, 0, sizeof(p));
    p.kind = kind;
    p.K = K;
    p.max_rounds = max_rounds;
    p.beta = beta;
    p.rtab = as_ptr<const float>(rtab);
    HIP_CHECK(fl_launch_robust(d, p, as_ptr<const float* const>(src), as_ptr<float* const>(dst), n_dst,
                               as_ptr<const FLState>(state), tails_len, as_stream(stream),
                               as_ptr<const unsigned long long>(keep)));
}

// Byzantine attack stage (fl_attack.hip) across engines' buffers, as robust_aggregate is: one launch rewrites, in
// place, the contributions of the bad sampled clients among the K buffers of the device table `src` (int64
// addresses).  `kind`: index in fedmi/fl/attack.py ATTACKS (1 sign_flip, 2 gauss, 3 alie, 4 ipm); `x`: the image
// the round trained from; `wtab`: [max_rounds, K] fp32 FedAvg weights of the buffers, 0 = all 1; `bad_mask`: bit k
// = client k is Byzantine.
static void attack_apply(std::vector<int> dims, int kind, double scale, double z, unsigned long long seed, uintptr_t src,
                         int K, uintptr_t x, uintptr_t wtab, unsigned long long bad_mask, uintptr_t state, uintptr_t rtab,
                         int max_rounds, uintptr_t stream) {
    const MLPDesc d = desc_of(dims, "attack_apply");
    if (kind < FL_ATTACK_SIGN_FLIP || kind > FL_ATTACK_IPM)
        throw std::runtime_error("attack_apply: kind must be 1 (sign_flip), 2 (gauss), 3 (alie) or 4 (ipm), got " +
                                 std::to_string(kind));
    if (K < 1 || K > FL_ATTACK_MAX_K)
        throw std::runtime_error("attack_apply: K must be 1.." + std::to_string(FL_ATTACK_MAX_K) +
                                 " clients (the width of the sampled-client mask), got " + std::to_string(K));
    const float sf = (float)scale, zf = (float)z;
    if (!(sf > 0.f) || !std::isfinite(sf)) throw std::runtime_error("attack_apply: scale must be finite and > 0 in fp32");
    if (!std::isfinite(zf)) throw std::runtime_error("attack_apply: z must be finite in fp32");
    if (K < 64 && (bad_mask >> K) != 0)
        throw std::runtime_error("attack_apply: bad_mask names a client >= K = " + std::to_string(K));
    if (max_rounds < 1) throw std::runtime_error("attack_apply: max_rounds must be >= 1");
    if (!src) throw std::runtime_error("attack_apply: src (the table of buffer addresses) is null");
    if (!x) throw std::runtime_error("attack_apply: x (the image the round trained from) is null");
    if (!state) throw std::runtime_error("attack_apply: state is null");
    if (!rtab) throw std::runtime_error("attack_apply: rtab is null");
    FLAttack p;
    std::memset(&p, 0, sizeof(p));
    p.kind = kind;
    p.K = K;
    p.max_rounds = max_rounds;
    p.scale = sf;
    p.z = zf;
    p.key0 = (uint32_t)seed;
    p.key1 = (uint32_t)(seed >> 32);
    p.bad = bad_mask;
    p.rtab = as_ptr<const float>(rtab);
    p.wtab = as_ptr<const float>(wtab);
    HIP_CHECK(fl_launch_attack(d, p, as_ptr<float* const>(src), as_ptr<const float>(x), as_ptr<const FLState>(state),
                               as_stream(stream)));
}

// Geometric-median aggregate (fl_geomed.hip) across engines' buffers, as robust_aggregate is: the iters + 1
// launches of the smoothed Weiszfeld iteration.  `scratch`: geomed_scratch_floats(dims, iters) caller-owned
// floats (distance partials, then one GEOMED_SLOT record per iteration: weights, distances, combined mask).
static void geomed_aggregate(std::vector<int> dims, int iters, double nu, uintptr_t src, int K, uintptr_t dst, int n_dst,
                             uintptr_t state, uintptr_t rtab, int tails_len, int max_rounds, uintptr_t scratch,
                             uintptr_t stream, uintptr_t keep) {
    const MLPDesc d = desc_of(dims, "geomed_aggregate");
    if (K < 1 || K > FL_GEOMED_MAX_K)
        throw std::runtime_error("geomed_aggregate: 1.." + std::to_string(FL_GEOMED_MAX_K) +
                                 " clients (the width of the sampled-client mask), got " + std::to_string(K));
    if (iters < 1 || iters > FL_GEOMED_MAX_ITERS)
        throw std::runtime_error("geomed_aggregate: iters must be in 1.." + std::to_string(FL_GEOMED_MAX_ITERS));
    const float nuf = (float)nu;
    if (!(nuf > 0.f) || !std::isfinite(nuf)) throw std::runtime_error("geomed_aggregate: nu must be finite and > 0 in fp32");
    if (n_dst < 1 || n_dst > FL_GEOMED_MAX_K || tails_len < 0 || max_rounds < 1 || !src || !dst || !state || !rtab ||
        !scratch)
        throw std::runtime_error("geomed_aggregate: bad arguments");
    FLGeomed p;
    std::memset(&p, 0, sizeof(p));
    p.K = K;
    p.max_rounds = max_rounds;
    p.rtab = as_ptr<const float>(rtab);
    p.T = iters;
    p.nu = nuf;
    HIP_CHECK(fl_launch_geomed(d, p, as_ptr<const float* const>(src), as_ptr<float* const>(dst), n_dst,
                               as_ptr<const FLState>(state), tails_len, as_ptr<float>(scratch), as_stream(stream),
                               as_ptr<const unsigned long long>(keep)));
}

// Multi-Krum screening (fl_screen.hip) across engines' buffers, as robust_aggregate is.  `src`: device table
// of K buffer addresses (int64); `dist`: K x K floats; `keep`: one uint64; `hist`: max_rounds uint64, all
// caller-owned; `f` / `m`: Byzantine clients assumed and clients kept (0: K_r - f).
static FLScreen screen_args(const char* who, int K, int f, int m, uintptr_t rtab, int max_rounds) {
    if (K < 1 || K > FL_SCREEN_MAX_K)
        throw std::runtime_error(std::string(who) + ": 1.." + std::to_string(FL_SCREEN_MAX_K) +
                                 " clients (the width of the sampled-client mask), got " + std::to_string(K));
    if (f < 0 || m < 0) throw std::runtime_error(std::string(who) + ": f and m must be >= 0");
    if (max_rounds < 1 || !rtab) throw std::runtime_error(std::string(who) + ": bad arguments");
    FLScreen p;
    std::memset(&p, 0, sizeof(p));
    p.K = K;
    p.f = f;
    p.m = m;
    p.max_rounds = max_rounds;
    p.rtab = as_ptr<const float>(rtab);
    return p;
}

static void screen_dist(std::vector<int> dims, uintptr_t src, int K, uintptr_t dist, uintptr_t state, uintptr_t rtab,
                        int max_rounds, uintptr_t stream, int tile) {
    const MLPDesc d = desc_of(dims, "screen_dist");
    const FLScreen p = screen_args("screen_dist", K, 0, 0, rtab, max_rounds);
    if (!src || !dist || !state) throw std::runtime_error("screen_dist: bad arguments");
    if (tile != 0 && tile != 1 && tile != 2 && tile != 4) throw std::runtime_error("screen_dist: tile must be 1, 2 or 4");
    HIP_CHECK(fl_launch_screen_dist(d, p, as_ptr<const float* const>(src), as_ptr<float>(dist),
                                    as_ptr<const FLState>(state), as_stream(stream), tile));
}

static void screen_select(uintptr_t dist, int K, int f, int m, uintptr_t keep, uintptr_t hist, uintptr_t state,
                          uintptr_t rtab, int max_rounds, uintptr_t stream) {
    const FLScreen p = screen_args("screen_select", K, f, m, rtab, max_rounds);
    if (!dist || !keep || !hist || !state) throw std::runtime_error("screen_select: bad arguments");
    HIP_CHECK(fl_launch_screen_select(p, as_ptr<const float>(dist), as_ptr<unsigned long long>(keep),
                                      as_ptr<unsigned long long>(hist), as_ptr<const FLState>(state),
                                      as_stream(stream)));
}

// Secure aggregation (fl_secagg.hip) across engines' buffers, as robust_aggregate is.  `bufs` / `clamp`:
// device tables of n buffer / uint32 [max_rounds] clamp-history addresses (int64) of clients
// first_client .. first_client + n - 1; `state` / `rtab`: a client's round state and per-round table.
static void secagg_mask(std::vector<int> dims, int bits, unsigned long long seed, uintptr_t bufs, int n,
                        int first_client, uintptr_t state, uintptr_t rtab, uintptr_t clamp, int max_rounds,
                        uintptr_t stream) {
    const MLPDesc d = desc_of(dims, "secagg_mask");
    if (bits < FL_SECAGG_MIN_BITS || bits > FL_SECAGG_MAX_BITS)
        throw std::runtime_error("secagg_mask: bits must be in 8 .. 30, got " + std::to_string(bits));
    if (n < 1 || first_client < 0 || first_client + n > FL_SECAGG_MAX_K)
        throw std::runtime_error("secagg_mask: clients 0.." + std::to_string(FL_SECAGG_MAX_K - 1) +
                                 " (the width of the sampled-client mask), got " + std::to_string(first_client) +
                                 " + " + std::to_string(n));
    if (max_rounds < 1 || !bufs || !state || !rtab || !clamp) throw std::runtime_error("secagg_mask: bad arguments");
    FLSecAgg p;
    std::memset(&p, 0, sizeof(p));
    p.bits = bits;
    p.first_client = first_client;
    p.max_rounds = max_rounds;
    p.key0 = (uint32_t)seed;
    p.key1 = (uint32_t)(seed >> 32);
    p.rtab = as_ptr<const float>(rtab);
    HIP_CHECK(fl_launch_secagg_mask(d, p, as_ptr<float* const>(bufs), n, as_ptr<uint32_t* const>(clamp),
                                    as_ptr<const FLState>(state), as_stream(stream)));
}

static void secagg_open(std::vector<int> dims, int bits, uintptr_t src, int K, uintptr_t dst, int n_dst,
                        uintptr_t state, uintptr_t rtab, int tails_len, int max_rounds, uintptr_t stream) {
    const MLPDesc d = desc_of(dims, "secagg_open");
    if (bits < FL_SECAGG_MIN_BITS || bits > FL_SECAGG_MAX_BITS)
        throw std::runtime_error("secagg_open: bits must be in 8 .. 30, got " + std::to_string(bits));
    if (K < 1 || K > FL_SECAGG_MAX_K)
        throw std::runtime_error("secagg_open: 1.." + std::to_string(FL_SECAGG_MAX_K) +
                                 " clients (the width of the sampled-client mask), got " + std::to_string(K));
    if (n_dst < 1 || n_dst > FL_SECAGG_MAX_K || tails_len < 0 || max_rounds < 1 || !src || !dst || !state || !rtab)
        throw std::runtime_error("secagg_open: bad arguments");
    FLSecAgg p;
    std::memset(&p, 0, sizeof(p));
    p.bits = bits;
    p.K = K;
    p.max_rounds = max_rounds;
    p.rtab = as_ptr<const float>(rtab);
    HIP_CHECK(fl_launch_secagg_open(d, p, as_ptr<const float* const>(src), as_ptr<float* const>(dst), n_dst,
                                    as_ptr<const FLState>(state), tails_len, as_stream(stream)));
}

// One fl_compress launch on caller-owned buffers of the image of `dims` (tests, tools): `residual` =
// 2 x Pimg floats (halves by round parity), `stat` = max_rounds floats, `state` / `rtab`: a client's
// round state and per-round table.
static void compress_launch(std::vector<int> dims, int kind, int k, bool error_feedback, uintptr_t local, uintptr_t x,
                            uintptr_t comm, uintptr_t residual, uintptr_t stat, uintptr_t state, uintptr_t rtab,
                            int max_rounds, uintptr_t stream, int levels, int client, unsigned long long seed) {
    const MLPDesc d = desc_of(dims, "compress_launch");
    if (kind < FL_COMPRESS_TOPK || kind > FL_COMPRESS_RANDK)
        throw std::runtime_error("compress_launch: kind must be 1 (topk), 2 (sign), 3 (qsgd) or 4 (randk)");
    if (kind == FL_COMPRESS_QSGD && (levels < 1 || levels > FL_COMPRESS_MAX_LEVELS))
        throw std::runtime_error("compress_launch: levels must be in 1 .. 32767");
    if (max_rounds < 1 || !local || !x || !comm || !residual || !stat || !state || !rtab)
        throw std::runtime_error("compress_launch: bad arguments");
    if (kind == FL_COMPRESS_SIGN || kind == FL_COMPRESS_QSGD) k = d.P;
    if (k < 1 || k > d.P) throw std::runtime_error("compress_launch: k must be in 1 .. P");
    FLCompress p;
    std::memset(&p, 0, sizeof(p));
    p.kind = kind;
    p.k = k;
    p.P = d.P;
    p.error_feedback = error_feedback ? 1 : 0;
    p.max_rounds = max_rounds;
    p.residual = as_ptr<float>(residual);
    p.stat_hist = as_ptr<float>(stat);
    p.levels = levels;
    p.client = client;
    p.key0 = (uint32_t)seed;
    p.key1 = (uint32_t)(seed >> 32);
    HIP_CHECK(fl_set_lds_limit_compress(d, kind));
    HIP_CHECK(fl_launch_compress(d, p, as_ptr<const float>(local), as_ptr<const float>(x), as_ptr<float>(comm),
                                 as_ptr<const FLState>(state), as_ptr<const float>(rtab), as_stream(stream)));
}

#ifndef FEDMI_SRC_DIGEST
#define FEDMI_SRC_DIGEST "unknown"
#endif
// found by fedmi/ops/build.py:so_digest in the file bytes (no load needed)
__attribute__((used)) static const char kSrcDigestMarker[] = "FEDMI_SRC_DIGEST:" FEDMI_SRC_DIGEST;

static py::dict device_info(int dev) {
    hipDeviceProp_t p;
    HIP_CHECK(hipGetDeviceProperties(&p, dev));
    py::dict o;
    o["name"] = std::string(p.name);
    o["arch"] = std::string(p.gcnArchName);
    o["cus"] = p.multiProcessorCount;
    o["lds_per_block"] = (long long)p.sharedMemPerBlock;
    o["hbm_bytes"] = (long long)p.totalGlobalMem;
    return o;
}

PYBIND11_MODULE(_fedmi_hip, m) {
    m.doc() = "fedmi native runtime: fused FL round kernels (gfx950), HIP graphs, RCCL";
    py::class_<RcclComm>(m, "RcclComm")
        .def(py::init<int, int, py::bytes, int, double>(), py::arg("nranks"), py::arg("rank"), py::arg("uid"),
             py::arg("device"), py::arg("timeout_s") = 120.0)
        .def_static("unique_id", &RcclComm::unique_id)
        .def("async_error", &RcclComm::async_error)
        .def("allreduce_f32", &RcclComm::allreduce_f32)
        .def("allreduce_f64", &RcclComm::allreduce_f64)
        .def("allreduce_bf16", &RcclComm::allreduce_bf16)
        .def("allgather_f32", &RcclComm::allgather_f32)
        .def("broadcast_bytes", &RcclComm::broadcast_bytes)
        .def("abort", &RcclComm::abort)
        .def("destroy", &RcclComm::destroy)
        .def_property_readonly("rank", &RcclComm::rank)
        .def_property_readonly("size", &RcclComm::size);
    py::class_<FLEngine>(m, "FLEngine")
        .def(py::init<std::vector<int>, py::dict, py::dict>())
        .def("run", &FLEngine::run, py::arg("r0"), py::arg("n"), py::arg("stream"), py::arg("comm") = nullptr,
             py::arg("close") = true)
        .def("run_local", &FLEngine::run_local)
        .def("phase", &FLEngine::phase, py::arg("r"), py::arg("which"), py::arg("stream"), py::arg("comm") = nullptr)
        .def("finalize", &FLEngine::finalize)
        .def("capture", &FLEngine::capture, py::arg("n"), py::arg("stream"), py::arg("comm") = nullptr)
        .def("replay", &FLEngine::replay)
        .def("flags", &FLEngine::flags)
        .def("set_flags", &FLEngine::set_flags)
        .def("graph_rounds", &FLEngine::graph_rounds)
        .def_property_readonly("graph_captures", &FLEngine::graph_captures)
        .def_property_readonly("eval_launches", &FLEngine::eval_launches)
        .def("time_kernels", &FLEngine::time_kernels)
        .def("trace", &FLEngine::trace, py::arg("r0"), py::arg("n"), py::arg("stream"), py::arg("comm") = nullptr,
             py::arg("close") = true, py::arg("gate_us") = 5000.0, py::arg("warm") = 0)
        .def("set_debug", &FLEngine::set_debug)
        .def("set_heldout", &FLEngine::set_heldout, py::arg("X"), py::arg("y"), py::arg("n"), py::arg("scratch"),
             py::arg("hist_cm"), py::arg("hist_loss"), py::arg("best_image"), py::arg("best"), py::arg("keep_best"))
        .def_property_readonly("heldout", &FLEngine::heldout)
        .def_property_readonly("heldout_rows_per_block", &FLEngine::heldout_rows_per_block)
        .def("predict", &FLEngine::predict, py::arg("X"), py::arg("n"), py::arg("params"), py::arg("proba"),
             py::arg("pred"), py::arg("stream"))
        .def("invalidate", &FLEngine::invalidate)
        .def("set_dp_seed", &FLEngine::set_dp_seed)
        .def("set_compress_seed", &FLEngine::set_compress_seed)
        .def("packed_global", &FLEngine::packed_global)
        .def("packed_local", &FLEngine::packed_local)
        .def("set_early_stop", &FLEngine::set_early_stop)
        .def("reset_pending", &FLEngine::reset_pending)
        .def("attach_peer", &FLEngine::attach_peer, py::keep_alive<1, 2>())
        .def_property_readonly("has_peer", &FLEngine::has_peer)
        .def("needs_eager_round", &FLEngine::needs_eager_round)
        .def_property_readonly("fused", &FLEngine::fused)
        .def_property_readonly("lagged", &FLEngine::lagged)
        .def_property_readonly("adam_exchange", &FLEngine::adam_exchange)
        .def_property_readonly("late_fold", &FLEngine::late_fold)
        .def("launch_one", &FLEngine::launch_one)
        .def("confusion", &FLEngine::confusion)
        .def("layout", &FLEngine::layout)
        .def("slab_map", &FLEngine::slab_map);
    py::class_<TrialBatch>(m, "TrialBatch")
        .def(py::init<std::vector<FLEngine*>>(), py::keep_alive<1, 2>())
        .def("run", &TrialBatch::run, py::arg("r0"), py::arg("n"), py::arg("stream"), py::arg("close") = true)
        .def("run_local", &TrialBatch::run_local)
        .def("finalize", &TrialBatch::finalize)
        .def("needs_eager_round", &TrialBatch::needs_eager_round)
        .def_property_readonly("size", &TrialBatch::size);
    m.def("synth", &synth, py::arg("X"), py::arg("y"), py::arg("n"), py::arg("F"), py::arg("seed"), py::arg("off"),
          py::arg("w1"), py::arg("w2"), py::arg("H"), py::arg("stream"), py::arg("label_noise") = 0.f);
    m.def("robust_aggregate", &robust_aggregate, py::arg("dims"), py::arg("kind"), py::arg("beta"), py::arg("src"),
          py::arg("K"), py::arg("dst"), py::arg("n_dst"), py::arg("state"), py::arg("rtab"), py::arg("tails_len"),
          py::arg("max_rounds"), py::arg("stream"), py::arg("keep") = (uintptr_t)0);
    m.def("attack_apply", &attack_apply, py::arg("dims"), py::arg("kind"), py::arg("scale"), py::arg("z"), py::arg("seed"),
          py::arg("src"), py::arg("K"), py::arg("x"), py::arg("wtab"), py::arg("bad_mask"), py::arg("state"),
          py::arg("rtab"), py::arg("max_rounds"), py::arg("stream"));
    m.attr("ATTACK_STREAM") = (unsigned)FL_ATTACK_STREAM;
    m.attr("ATTACK_MAX_K") = (int)FL_ATTACK_MAX_K;
    m.def("geomed_aggregate", &geomed_aggregate, py::arg("dims"), py::arg("iters"), py::arg("nu"), py::arg("src"),
          py::arg("K"), py::arg("dst"), py::arg("n_dst"), py::arg("state"), py::arg("rtab"), py::arg("tails_len"),
          py::arg("max_rounds"), py::arg("scratch"), py::arg("stream"), py::arg("keep") = (uintptr_t)0);
    m.def("geomed_scratch_floats", [](const std::vector<int>& dims, int iters) {
        return fl_geomed_scratch_floats(desc_of(dims, "geomed_scratch_floats").Pimg, iters);
    });
    m.attr("GEOMED_SLOT") = (int)FL_GEOMED_SLOT;
    m.attr("GEOMED_THREADS") = (int)FL_GEOMED_THREADS;
    m.attr("GEOMED_MAX_ITERS") = (int)FL_GEOMED_MAX_ITERS;
    m.def("screen_dist", &screen_dist, py::arg("dims"), py::arg("src"), py::arg("K"), py::arg("dist"), py::arg("state"),
          py::arg("rtab"), py::arg("max_rounds"), py::arg("stream"), py::arg("tile") = 0);
    m.def("screen_select", &screen_select, py::arg("dist"), py::arg("K"), py::arg("f"), py::arg("m"), py::arg("keep"),
          py::arg("hist"), py::arg("state"), py::arg("rtab"), py::arg("max_rounds"), py::arg("stream"));
    m.def("compress_launch", &compress_launch, py::arg("dims"), py::arg("kind"), py::arg("k"),
          py::arg("error_feedback"), py::arg("local"), py::arg("x"), py::arg("comm"), py::arg("residual"),
          py::arg("stat"), py::arg("state"), py::arg("rtab"), py::arg("max_rounds"), py::arg("stream"),
          py::arg("levels") = 127, py::arg("client") = 0, py::arg("seed") = 0ull);
    m.def("secagg_mask", &secagg_mask, py::arg("dims"), py::arg("bits"), py::arg("seed"), py::arg("bufs"), py::arg("n"),
          py::arg("first_client"), py::arg("state"), py::arg("rtab"), py::arg("clamp"), py::arg("max_rounds"),
          py::arg("stream"));
    m.def("secagg_open", &secagg_open, py::arg("dims"), py::arg("bits"), py::arg("src"), py::arg("K"), py::arg("dst"),
          py::arg("n_dst"), py::arg("state"), py::arg("rtab"), py::arg("tails_len"), py::arg("max_rounds"),
          py::arg("stream"));
    m.attr("SECAGG_STREAM") = (unsigned)FL_SECAGG_STREAM;
    m.attr("QSGD_STREAM") = (unsigned)FL_QSGD_STREAM;
    m.attr("RANDK_STREAM") = (unsigned)FL_RANDK_STREAM;
    m.attr("ROBUST_MAX_K") = (int)FL_ROBUST_MAX_K;
    m.attr("HELDOUT_MAX_ROWS") = (int)FL_HELDOUT_MAX_ROWS;
    m.def("device_info", &device_info);
    m.attr("STATE_BYTES") = (int)sizeof(FLState);
    // floats per slab row an engine of this model may need at R rows per workgroup: the dense row, or the
    // longer blocked row where the engine may choose it (the caller sizes the slab before it constructs
    // the engine and passes the size as bufs["slab_floats"])
    m.def("slab_row_floats", [](const std::vector<int>& dims, int R) {
        int P = 0;
        for (size_t l = 0; l + 1 < dims.size(); ++l) P += dims[l] * dims[l + 1] + dims[l + 1];
        const MLPDesc rd = FlRefShape<32>::d;
        bool ref = R == 32 && (int)dims.size() == rd.L + 1;
        for (int l = 0; ref && l <= rd.L; ++l) ref = dims[l] == rd.dim[l];
        return (((ref ? std::max(P, FlRefSlabBlk<32>::s.P) : P) + 1) + 3) & ~3;
    });
    m.attr("SRC_DIGEST") = std::string(kSrcDigestMarker + sizeof("FEDMI_SRC_DIGEST:") - 1);
    register_trainer(m);
    register_peer(m);
}
