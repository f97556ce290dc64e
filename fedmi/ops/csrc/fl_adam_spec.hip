// Shape-specialised Adam kernel for the reference 14-50-200-2 MLP at R = 32, rounds without an
// in-kernel exchange, in a translation unit of its own (as fl_train_bf16_spec.hip).  The body is the
// generic kernel's (fl_adam_body.inc), so every value is the same computation in the same order
// (tests/test_adam_spec.py: bitwise), with
//   * the descriptors bound to the compile-time constants of FlRefShape<32> (fl_layout.h): the map
//     from dense index to image / packed position (fl_adam_map.h) divides by the constants 14, 50
//     and 200 and adds immediates;
//   * one compact argument struct (FlAdamSpecArgs, fl_common.h) instead of MLPDesc, FLConfig,
//     FLBuffers and MLPDescB by value: pointers first, then the optimizer scalars, the early-stop
//     scalars of the fold last.  The FLConfig / FLBuffers the body reads are rebuilt from it in
//     registers; one client, no lag region, no undo buffer and no exchange are constants, so those
//     paths are compiled out (fl_adam_spec_ok keeps the kernel away from rounds where one is live);
//   * the double-precision metric fold (fl_device.h finalize_state) out of line, behind the
//     fold_may_stop / block-0 test of round_state: same arithmetic, on every block whenever
//     fold_may_stop holds, but not in the parameter blocks' straight-line code;
//   * the round state loaded by wave 0 with the kernel's first instructions and the step's sched
//     entries fetched together with its rtab entry (fl_adam_body.inc ADAM_EARLY): the two dependent
//     trips to memory end before the slab sums do instead of after them;
//   * engine (packed bf16 image or not) and slab format as template parameters.
// Measured in profiles/adam_floor_stamps.log and profiles/adam_spec_ab.log.
#include "fl_common.h"
#include "fl_device.h"
#include "fl_layout.h"
#include "peer_device.h"
#include "fl_adam.h"

static_assert(sizeof(FlAdamSpecArgs) == 224, "FlAdamSpecArgs: three and a half 64-byte lines");

// The metric fold of round_state, called by the whole of wave 0: folds the state at `st` and leaves
// the result (lane 0's: fl_device.h fold_round) at `out`, the block's LDS copy of the state.  Scalars
// and pointers only: a reference to the kernel's rebuilt FLConfig, or an FLState by value, would
// put that struct into scratch on the parameter blocks' path too.
static __device__ __noinline__ void fl_adam_spec_fold(double* hist_global, double* hist_rank, float* hist_loss,
                                                      const float* rtab, const float* anchor, double atol, double rtol,
                                                      int patience, int metric_mode, int es_enabled, int max_rounds,
                                                      int fold_mask, bool write_hist, const FLState* st, FLState* out) {
    constexpr MLPDesc d = FlRefShape<32>::d;
    FLConfig c = {};
    c.world = 1;
    c.tail_off = d.Pimg;
    c.tail_stride = d.dim[d.L] * d.dim[d.L] + 1;
    c.tail_len = c.tail_stride;
    c.max_rounds = max_rounds;
    c.metric_mode = metric_mode;
    c.es_enabled = es_enabled;
    c.patience = patience;
    c.atol = atol;
    c.rtol = rtol;
    FLBuffers b = {};
    b.hist_global = hist_global;
    b.hist_rank = hist_rank;
    b.hist_loss = hist_loss;
    b.rtab = rtab;
    const FLState S = finalize_state(d, c, b, anchor, *st, write_hist, fold_mask);
    if ((threadIdx.x & 63) == 0) *out = S;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // stored before the caller reads it back
}
__device__ __forceinline__ FLState fl_adam_spec_folded(const FlAdamSpecArgs& a, const float* anchor, int fold_mask,
                                                       bool write_hist, const FLState* st, FLState* sh) {
    fl_adam_spec_fold(a.hist_global, a.hist_rank, a.hist_loss, a.rtab, anchor, a.atol, a.rtol, a.patience,
                      a.metric_mode, a.es_enabled, a.max_rounds, fold_mask, write_hist, st, sh);
    // field by field: after a whole-struct copy the compiler keeps `prev` as a per-thread array and
    // promotes it to LDS, indexed through the workgroup size it reads from the dispatch packet -- a
    // load from host memory in every wave
    FLState r;
    r.next_round = sh->next_round;
    r.finalized = sh->finalized;
    r.stopped = sh->stopped;
    r.live = sh->live;
    r.cur_round = sh->cur_round;
    r.count = sh->count;
    r.has_prev = sh->has_prev;
    r.stop_round = sh->stop_round;
    r.calls = sh->calls;
    r.late = sh->late;
#pragma unroll
    for (int q = 0; q < 4; ++q) r.prev[q] = sh->prev[q];
    return r;
}

// BLK (fp16 slab only): the slab rows are blocked rows (fl_layout.h FlSlabBlk, written by the blocked
// instantiation of fl_train_bf16_spec.hip).  A block owns 64 consecutive row positions instead of 64
// dense indices -- a few more blocks -- and maps each to its dense index (a pad column: an idle lane)
// before fl_adam_pos; the row reduction is the body's, so every parameter's partials are added in the
// same order as from dense rows.  Pads hold zeros: the saturation flag never sees them fire.
template <int PACK, int SLAB_F16, bool BLK = false>
__global__ void __launch_bounds__(ADAM_WAVES * 64) fl_adam_spec_kernel(FlAdamSpecArgs a) {
    static_assert(!BLK || SLAB_F16, "the blocked row is an fp16 row");
    constexpr MLPDesc d = FlRefShape<32>::d;  // (local copies: folded, fl_layout.h FL_SHAPE_D)
    constexpr MLPDescB e = FlRefShape<32>::e;
    constexpr FlSlabBlk sb = FlRefSlabBlk<32>::s;
    constexpr int pack = PACK;
    FLConfig c = {};
    c.R = 32;
    c.world = 1;
    c.inv_n = a.inv_n;
    c.slab_stride = a.slab_stride;
    c.n_slabs = a.n_slabs;
    c.slab_f16 = SLAB_F16;
    c.tail_off = d.Pimg;
    c.tail_stride = d.dim[d.L] * d.dim[d.L] + 1;
    c.tail_len = c.tail_stride;
    c.local_steps = a.local_steps;
    c.omb1 = a.omb1;
    c.omb2 = a.omb2;
    c.beta2f = a.beta2f;
    c.eps = a.eps;
    c.weight_decay = a.weight_decay;
    c.prox_mu = a.prox_mu;
    c.es_enabled = a.es_enabled;
    c.max_rounds = a.max_rounds;
    FLBuffers b = {};
    b.slab = a.slab;
    b.local = a.local;
    b.m = a.m;
    b.v = a.v;
    b.dbg = a.dbg;
    b.pk_local = a.pk_local;
    b.sched = a.sched;
    b.rtab = a.rtab;
    b.sat = a.sat;
    const float* __restrict__ pin = a.pin;
    const float* __restrict__ anchor = a.anchor;
    float* __restrict__ comm = a.comm;
    const FLState* __restrict__ st = a.st;
    FLState* __restrict__ st_out = a.st_out;
    const int local_step = a.local_step, fold = a.fold, tail_a = a.tail_a, fold_mask = a.fold_mask;
    const PeerArgs pa = {};
    const int xchg = 0, afold = 0;
#define ADAM_PA_LL false
#define ADAM_STATIC true
#define ADAM_EARLY 1
// (S0 is still the state at `st` where round_state folds; S_sh: the body's LDS copy, which wave 0
// alone writes before the block's barrier)
#define ADAM_FINALIZE(S0, hist) fl_adam_spec_folded(a, anchor, fold_mask, hist, st, &S_sh)
#define ADAM_SLAB_LEN (BLK ? sb.P : d.P)
#define ADAM_SLAB_DENSE(p) (BLK ? fl_slab_blk_dense(d, sb, (p)) : (p))
#define ADAM_SLAB_VALID(di) (BLK ? (di) >= 0 : (di) < d.P)
#include "fl_adam_body.inc"
#undef ADAM_SLAB_VALID
#undef ADAM_SLAB_DENSE
#undef ADAM_SLAB_LEN
#undef ADAM_FINALIZE
#undef ADAM_EARLY
#undef ADAM_STATIC
#undef ADAM_PA_LL
}

// One client, no lag region, no undo buffer, descriptors byte-equal to the constants (an fp32 engine
// has no MLPDescB: `e` null), and the engine / slab pair is instantiated.
bool fl_adam_spec_ok(const MLPDesc& d, const MLPDescB* e, const FLConfig& c, const FLBuffers& b) {
    const MLPDesc rd = FlRefShape<32>::d;
    const int ts = rd.dim[rd.L] * rd.dim[rd.L] + 1;
    if (c.R != 32 || c.world != 1 || c.rank != 0 || c.lag_off != 0 || b.undo != nullptr) return false;
    if (c.tail_off != rd.Pimg || c.tail_stride != ts || c.tail_len != ts) return false;
    if (e == nullptr) return !c.slab_f16 && std::memcmp(&d, &rd, sizeof(d)) == 0;
    return fl_ref_shape_match<32>(d, *e);
}

hipError_t fl_launch_adam_spec(const FLConfig& c, const FLBuffers& b, const float* pin, const float* anchor,
                               float* comm, const FLState* st, int local_step, int pack, FLState* st_out, int fold,
                               int tail_a, int fold_mask, hipStream_t s, bool slab_blocked) {
    if (!pack && c.slab_f16) return hipErrorInvalidValue;
    if (slab_blocked && (!c.slab_f16 || c.slab_stride < FlRefSlabBlk<32>::s.P + 1)) return hipErrorInvalidValue;
    FlAdamSpecArgs a = {};
    a.pin = pin;
    a.anchor = anchor;
    a.comm = comm;
    a.st = st;
    a.slab = b.slab;
    a.local = b.local;
    a.m = b.m;
    a.v = b.v;
    a.sched = b.sched;
    a.rtab = b.rtab;
    a.pk_local = b.pk_local;
    a.sat = b.sat;
    a.dbg = b.dbg;
    a.st_out = st_out;
    a.hist_global = b.hist_global;
    a.hist_rank = b.hist_rank;
    a.hist_loss = b.hist_loss;
    a.n_slabs = c.n_slabs;
    a.slab_stride = c.slab_stride;
    a.local_steps = c.local_steps;
    a.max_rounds = c.max_rounds;
    a.local_step = local_step;
    a.fold = fold;
    a.tail_a = tail_a;
    a.fold_mask = fold_mask;
    a.inv_n = c.inv_n;
    a.omb1 = c.omb1;
    a.omb2 = c.omb2;
    a.beta2f = c.beta2f;
    a.eps = c.eps;
    a.weight_decay = c.weight_decay;
    a.prox_mu = c.prox_mu;
    a.es_enabled = c.es_enabled;
    a.patience = c.patience;
    a.metric_mode = c.metric_mode;
    a.atol = c.atol;
    a.rtol = c.rtol;
    const int blocks = ((slab_blocked ? FlRefSlabBlk<32>::s.P : FlRefShape<32>::d.P) + 63) / 64 + 1;
    const dim3 grid(blocks), block(ADAM_WAVES * 64);
    if (slab_blocked) hipLaunchKernelGGL((fl_adam_spec_kernel<1, 1, true>), grid, block, 0, s, a);
    else if (pack && c.slab_f16) hipLaunchKernelGGL((fl_adam_spec_kernel<1, 1>), grid, block, 0, s, a);
    else if (pack) hipLaunchKernelGGL((fl_adam_spec_kernel<1, 0>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((fl_adam_spec_kernel<0, 0>), grid, block, 0, s, a);
    return hipGetLastError();
}
