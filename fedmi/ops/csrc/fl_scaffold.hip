// SCAFFOLD (Karimireddy et al. 2020, "Stochastic Controlled Averaging for Federated Learning"), option I:
// control-variate drift correction of the local steps.  Client i keeps a control variate c_i, every replica
// the server variate c, both P floats in dense slab order (position p = dense parameter p), both 0 at start.
// In a live round r in which the client is sampled:
//
//   g0     = grad f_i(x), the full-batch gradient at the image the round trains from: the column sums of
//            the slab rows local step 0's train launch wrote (already scaled by 1 / n)
//   Adam sees g + (c - c_i) in every local step of the round, c and c_i as they were at the round's start
//   cnew_i = g0, delta_i = sub(cnew_i, c_i)                                       (pending until the fold)
//   after the model's aggregation: s = left fold from +0, in client order, of delta_j over the round's
//   sampled clients; c = add(c, div(s, float(N))), N the number of clients; c_i = add(c_i, delta_i) for the
//   sampled ones
//
// The commit is the addition c takes, not a copy of cnew_i: add(c_i, sub(g0, c_i)) is g0 only where the subtraction
// is exact, so a copy would leave c and the c_i one rounding apart after the first round even where every client
// holds the same shard.  Committed this way c and c_i move by the same operations: on equal shards with a power-of-two
// client count c == c_i bit for bit, the correction row is exact +0, and the round is the plain round's bit for bit.
// c_i stays within one rounding of g0 (the error does not accumulate: every round's delta is taken from g0 anew).
//
// Two kernels, every operation one round-to-nearest fp32 intrinsic in one fixed order (compiled without the
// packed fp32 forms, fedmi/ops/build.py), so fedmi/fl/scaffold.py reproduces both bit for bit.
//
// fl_scaffold_capture_kernel: one launch per round between local step 0's train and Adam launches.  It
// reduces slab rows [0, n_blk) -- the bytes the Adam kernel reads next -- and writes one more slab row, row
// n_blk = c - c_i, which every Adam kernel of the round then reduces like any other row (the engine gives
// the Adam launches n_blk + 1 rows and the train launches n_blk workgroups, so no train launch of a later
// local step overwrites it).  Work split: a 256-thread workgroup owns 64 consecutive positions; thread
// (q = tid & 15, r = tid >> 4) owns float4 q of them and rows r, r + 16, r + 32, ..., added in ascending row
// order from +0 with 16-byte loads, four row groups in flight before the first add; the 16 row partials of
// a position meet in a [16][64] LDS tile and threads 0-63 add them in r order from +0.  The order depends
// on n_blk and the position only.  Threads 0-63 store cnew, delta and the correction row; the correction
// row's floats [P, slab_stride) -- the loss slot at P among them, which the Adam kernel's tail block sums
// over all rows -- are written as exact 0.
//
// The gate.  The launch sits in front of the round's first Adam kernel, which folds the previous round's
// metrics and only then publishes the round's state; like the train kernel beside it, the capture works on
// the tentative decision of the round's INPUT state: live = not stopped and next_round < max_rounds, round
// = next_round.  A round the fold then finds stopped has pending values written that nothing reads: the
// fold kernel commits under the published state, and the next live round rewrites all of them.  A round
// that is not (tentatively) live, or in which this client is not sampled (rtab weight 0), writes nothing.
//
// fl_scaffold_fold_kernel<KB>: one thread per position, the K buckets of fl_robust (4 / 8 / 16 / 32 / 64),
// every delta load issued before the first use (fl_src_load<KB, 1>).  Unsampled clients are selected out
// by the round's mask, never multiplied by 0 (an inf or NaN they hold stays out).  The new c goes to all
// n_dst replicas (read from the first, which may be a destination: nobody else touches the position), and
// the n_own clients the launch owns (clients first_own ..) commit c_i = add(c_i, delta_i) when sampled.  A state
// that is not live returns at once.  No atomics, no grid barrier, plain vector stores.
#include "fl_common.h"
#include "fl_image.h"

#define FL_SCAFFOLD_THREADS 256
#define FL_SCAFFOLD_COLS 64      // positions per workgroup of the capture kernel
#define FL_SCAFFOLD_ROWS 16      // row partials per position: thread r takes rows r, r + 16, ...
#define FL_SCAFFOLD_DEPTH 4      // row groups in flight before the first add
#define FL_SCAFFOLD_FOLD_THREADS 64

__device__ __forceinline__ float4 scaffold_add4(float4 a, const float4 x) {
    a.x = __fadd_rn(a.x, x.x); a.y = __fadd_rn(a.y, x.y); a.z = __fadd_rn(a.z, x.z); a.w = __fadd_rn(a.w, x.w);
    return a;
}

__global__ void __launch_bounds__(FL_SCAFFOLD_THREADS)
fl_scaffold_capture_kernel(FLScaffold p, float* __restrict__ slab, const FLState* __restrict__ st) {
    __shared__ __attribute__((aligned(16))) float part[FL_SCAFFOLD_ROWS][FL_SCAFFOLD_COLS];
    // the train kernel's tentative decision on the round's input state (see the header)
    if (st->stopped || st->next_round < 0 || st->next_round >= p.max_rounds) return;
    if (fl_round_weight(p.rtab, st->next_round) == 0.f) return;
    const int tid = threadIdx.x, q = tid & 15, r = tid >> 4;
    const int p0 = (int)blockIdx.x * FL_SCAFFOLD_COLS + 4 * q;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    // (a row holds slab_stride floats, a multiple of 4: a float4 that starts inside a row ends inside it)
    if (p0 < p.slab_stride) {
        const float* col = slab + p0;
        const size_t rs = (size_t)p.slab_stride;
        int row = r;
        for (; row + (FL_SCAFFOLD_DEPTH - 1) * FL_SCAFFOLD_ROWS < p.n_blk; row += FL_SCAFFOLD_DEPTH * FL_SCAFFOLD_ROWS) {
            float4 x[FL_SCAFFOLD_DEPTH];
#pragma unroll
            for (int u = 0; u < FL_SCAFFOLD_DEPTH; ++u)
                x[u] = *reinterpret_cast<const float4*>(col + (size_t)(row + u * FL_SCAFFOLD_ROWS) * rs);
#pragma unroll
            for (int u = 0; u < FL_SCAFFOLD_DEPTH; ++u) acc = scaffold_add4(acc, x[u]);
        }
        for (; row < p.n_blk; row += FL_SCAFFOLD_ROWS)
            acc = scaffold_add4(acc, *reinterpret_cast<const float4*>(col + (size_t)row * rs));
    }
    *reinterpret_cast<float4*>(&part[r][4 * q]) = acc;
    __syncthreads();
    if (tid >= FL_SCAFFOLD_COLS) return;
    const int pos = (int)blockIdx.x * FL_SCAFFOLD_COLS + tid;
    if (pos >= p.slab_stride) return;
    float* corr = slab + (size_t)p.n_blk * p.slab_stride;
    if (pos >= p.P) {  // the loss slot and the row's padding
        corr[pos] = 0.f;
        return;
    }
    float g = 0.f;
#pragma unroll
    for (int k = 0; k < FL_SCAFFOLD_ROWS; ++k) g = __fadd_rn(g, part[k][tid]);
    const float ci = p.ci[pos];
    p.cnew[pos] = g;
    p.delta[pos] = __fsub_rn(g, ci);
    corr[pos] = __fsub_rn(p.c[pos], ci);
}

hipError_t fl_launch_scaffold_capture(const FLScaffold& p, float* slab, const FLState* st, hipStream_t s) {
    if (p.P < 1 || p.n_blk < 1 || p.slab_stride <= p.P || (p.slab_stride & 3) != 0 || p.max_rounds < 1 ||
        p.rtab == nullptr || p.c == nullptr || p.ci == nullptr || p.cnew == nullptr || p.delta == nullptr ||
        slab == nullptr || st == nullptr || ((uintptr_t)slab & 15) != 0)
        return hipErrorInvalidValue;
    const int blocks = (p.slab_stride + FL_SCAFFOLD_COLS - 1) / FL_SCAFFOLD_COLS;
    hipLaunchKernelGGL(fl_scaffold_capture_kernel, dim3(blocks), dim3(FL_SCAFFOLD_THREADS), 0, s, p, slab, st);
    return hipGetLastError();
}

template <int KB>
__global__ void __launch_bounds__(FL_SCAFFOLD_FOLD_THREADS)
fl_scaffold_fold_kernel(FLScaffold p, const float* const* __restrict__ src, float* const* __restrict__ dst, int n_dst,
                        float* const* __restrict__ ci, int n_own, int first_own, const FLState* __restrict__ st) {
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;
    const int pos = (int)blockIdx.x * FL_SCAFFOLD_FOLD_THREADS + threadIdx.x;
    if (pos >= p.P) return;
    float v[KB][1];
    fl_src_load<KB, 1>(src, p.K, 0, pos, v);
    const float c_old = dst[0][pos];
    const uint64_t mask = fl_round_mask(p.rtab, r, p.K);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < KB; ++i) sum = (i < p.K && ((mask >> i) & 1ull)) ? __fadd_rn(sum, v[i][0]) : sum;
    const float c_new = __fadd_rn(c_old, __fdiv_rn(sum, (float)p.N));
    for (int k = 0; k < n_dst; ++k) dst[k][pos] = c_new;
    // (the owned clients' deltas are the ones loaded above: compile-time slots, no second load)
#pragma unroll
    for (int i = 0; i < KB; ++i)
        if (i >= first_own && i < first_own + n_own && ((mask >> i) & 1ull)) {
            float* own = ci[i - first_own];
            own[pos] = __fadd_rn(own[pos], v[i][0]);
        }
}

template <int KB>
static void scaffold_fold_launch(const FLScaffold& p, const float* const* src, float* const* dst, int n_dst,
                                 float* const* ci, int n_own, int first_own, const FLState* st, hipStream_t s) {
    const int blocks = (p.P + FL_SCAFFOLD_FOLD_THREADS - 1) / FL_SCAFFOLD_FOLD_THREADS;
    hipLaunchKernelGGL(fl_scaffold_fold_kernel<KB>, dim3(blocks), dim3(FL_SCAFFOLD_FOLD_THREADS), 0, s, p, src, dst,
                       n_dst, ci, n_own, first_own, st);
}

hipError_t fl_launch_scaffold_fold(const FLScaffold& p, const float* const* src, float* const* dst, int n_dst,
                                   float* const* ci, int n_own, int first_own, const FLState* st, hipStream_t s) {
    if (p.P < 1 || p.K < 1 || p.K > FL_SCAFFOLD_MAX_K || p.N < 1 || p.max_rounds < 1 || p.rtab == nullptr ||
        src == nullptr || dst == nullptr || n_dst < 1 || n_own < 0 || first_own < 0 || first_own + n_own > p.K ||
        (n_own > 0 && ci == nullptr) || st == nullptr)
        return hipErrorInvalidValue;
    if (p.K <= 4) scaffold_fold_launch<4>(p, src, dst, n_dst, ci, n_own, first_own, st, s);
    else if (p.K <= 8) scaffold_fold_launch<8>(p, src, dst, n_dst, ci, n_own, first_own, st, s);
    else if (p.K <= 16) scaffold_fold_launch<16>(p, src, dst, n_dst, ci, n_own, first_own, st, s);
    else if (p.K <= 32) scaffold_fold_launch<32>(p, src, dst, n_dst, ci, n_own, first_own, st, s);
    else scaffold_fold_launch<64>(p, src, dst, n_dst, ci, n_own, first_own, st, s);
    return hipGetLastError();
}
