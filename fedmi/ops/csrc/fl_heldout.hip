// Held-out scoring of the aggregated model inside the round, and row-wise inference.
//
// Every robust rule, screen, DP noise, compressor and server optimizer changes the AGGREGATED model,
// while the round's own metrics score each client's local post-step model on its training shard.
// These two launches, issued after a round's aggregation (and server step), score the round's output
// image on a caller-supplied held-out set without leaving the stream or the captured graph:
//
//   fl_heldout_rows_kernel<RT> : one workgroup per R = 16 RT rows.  Forward-only, fp32: the device
//       functions of fl_kernels.hip (stage_image, stage_rows, forward_block: the exact f32 MFMA
//       chain of the evaluation kernel), then per row the first-maximum argmax of the logits
//       (eval_rows' rule and addressing) and the softmax cross-entropy lse(z) - z[y] with the
//       maximum subtracted.  It reads the fp32 master image for fp32 and bf16 engines alike, as the
//       stand-alone confusion launch does.
//         reduce mode: gated by the state of the round's output parity (fl_round_gate); writes ONE
//           partial per workgroup -- C x C int32 counts and the fp32 sum of its rows' losses, added
//           in row order by one thread -- to scratch[blk] with plain stores.  Rows >= n add nothing.
//           No float atomics, nothing to zero between rounds.
//         row mode: ungated; writes proba[row][0..C) (the fp32 softmax) and / or pred[row] (the
//           argmax of the LOGITS) for rows < n.
//   fl_heldout_fold_kernel : one workgroup of T = 1024 threads, same gate.  Thread t adds partials t,
//       t + T, ... in that order, then block_sum_ordered: one canonical order whatever ran the row
//       launch.  Counts are integer sums.  Writes round r's row of the device history (counts, fp32 loss SUM); with
//       keep_best, `loss_sum < best` under a plain < copies the round's image into best_image and
//       records the round: NaN never wins, ties keep the earlier round.
//
// The round comes from the state, as in fl_server.hip: no per-round host argument, both launches
// capture into the round graphs.
#define FL_FP32_DEVICE_ONLY
#include "fl_kernels.hip"
#include "fl_image.h"

// static LDS of the row kernel: C x C counters, then one loss per row (a multiple of 16 bytes, so
// the dynamic window behind it keeps its alignment)
#define FL_HO_STATIC_INTS (FL_MAX_CLASSES * FL_MAX_CLASSES + 32)

template <int RT>
__global__ void __launch_bounds__(FL_THREADS)
fl_heldout_rows_kernel(MLPDesc d, FLHeldout h, const float* __restrict__ params, const FLState* __restrict__ st,
                       float* __restrict__ proba, int* __restrict__ pred) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ __attribute__((aligned(16))) int ho_s[FL_HO_STATIC_INTS];
    const bool rows_out = proba != nullptr || pred != nullptr;
    if (!rows_out) {
        int r;
        if (!fl_round_gate(st, h.max_rounds, r)) return;
    }
    constexpr int R = RT * 16;
    const int row0 = blockIdx.x * R;
    const int C = d.dim[d.L];
    int* cm_s = ho_s;
    float* loss_s = reinterpret_cast<float*>(ho_s + FL_MAX_CLASSES * FL_MAX_CLASSES);
    float* acts = lds;
    float* li = lds + d.img_lds;
    for (int e = threadIdx.x; e < C * C; e += FL_THREADS) cm_s[e] = 0;
    // labels are needed only after the forward pass: issue the load now
    const int ylab = (!rows_out && threadIdx.x < R) ? h.y[min(row0 + (int)threadIdx.x, h.n - 1)] : 0;
    stage_image(d, params, li);
    stage_rows<RT>(h.X, h.n, d.dim[0], row0, acts + d.act_off[0], d.ld[0]);
    lds_barrier();
    forward_block<RT>(d, acts, li);
    if (threadIdx.x < R) {
        const int r = threadIdx.x, row = row0 + r;
        float loss = 0.f;
        if (row < h.n) {
            const float* zr = acts + d.act_off[d.L] + r * d.ld[d.L];
            const int sr = fl_swz(r);
            int best = 0;
            float bv = zr[sr];
            for (int k = 1; k < C; ++k)
                if (zr[k ^ sr] > bv) { bv = zr[k ^ sr]; best = k; }
            // softmax denominator around the maximum (bv: NaN logits leave it at z[0], the sum is NaN then)
            float se = 0.f;
            for (int k = 0; k < C; ++k) se = __fadd_rn(se, expf(__fsub_rn(zr[k ^ sr], bv)));
            if (rows_out) {
                if (pred != nullptr) pred[row] = best;
                if (proba != nullptr)
                    for (int k = 0; k < C; ++k) proba[(size_t)row * C + k] = expf(__fsub_rn(zr[k ^ sr], bv)) / se;
            } else if ((unsigned)ylab < (unsigned)C) {
                loss = __fsub_rn(__fadd_rn(bv, logf(se)), zr[ylab ^ sr]);
                atomicAdd(&cm_s[ylab * C + best], 1);
            }
        }
        loss_s[r] = loss;
    }
    if (rows_out) return;
    lds_barrier();
    int* out = h.scratch + (size_t)blockIdx.x * (C * C + 1);
    for (int e = threadIdx.x; e < C * C; e += FL_THREADS) out[e] = cm_s[e];
    if (threadIdx.x == 0) {
        float s = 0.f;  // one fixed order: the block's rows from the first to the last
#pragma unroll
        for (int r = 0; r < R; ++r) s = __fadd_rn(s, loss_s[r]);
        out[C * C] = __float_as_int(s);
    }
}

// (latency-bound: one workgroup, a few hundred partials.  Every global load -- the best sum so far, the
// loss partials, the count partials -- is issued before the first is used, the counts as one flat
// (partial, cell) index space over all 1024 threads; measured with the loads cell after cell on 256
// threads: 13.0 us per launch against 10.3 us for the row kernel, profiles/heldout_trace.jsonl.)
__global__ void __launch_bounds__(FL_HELDOUT_FOLD_THREADS)
fl_heldout_fold_kernel(MLPDesc d, FLHeldout h, int n_blk, const float* __restrict__ image,
                       const FLState* __restrict__ st) {
    constexpr int T = FL_HELDOUT_FOLD_THREADS, W = T / 64, CCMAX = FL_MAX_CLASSES * FL_MAX_CLASSES;
    __shared__ int cm_w[W * CCMAX];  // one set of counters per wave: same-cell atomics only collide inside a wave
    __shared__ float wsum[W];
    int r;
    if (!fl_round_gate(st, h.max_rounds, r)) return;
    const int C = d.dim[d.L], CC = C * C, stride = CC + 1;
    const int t = threadIdx.x, wave = t >> 6;
    for (int e = t; e < W * CC; e += T) cm_w[e] = 0;
    __syncthreads();
    const float cur = h.keep_best ? h.best[0] : 0.f;  // (read by every thread before thread 0 may replace it)
    // loss: partials t, t + T, ... in that order, then the workgroup's one fixed order
    float acc = 0.f;
    for (int p = t; p < n_blk; p += T) acc = __fadd_rn(acc, __int_as_float(h.scratch[(size_t)p * stride + CC]));
    // counts: integer LDS atomics (exact in any order)
    for (int idx = t; idx < n_blk * CC; idx += T) {
        const int p = idx / CC, e = idx - p * CC;
        const int v = h.scratch[(size_t)p * stride + e];
        if (v) atomicAdd(&cm_w[wave * CC + e], v);
    }
    const float sum = block_sum_ordered<T>(acc, wsum);  // (its barrier also completes the count atomics)
    for (int e = t; e < CC; e += T) {
        int a = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) a += cm_w[w * CC + e];
        h.hist_cm[(size_t)r * CC + e] = a;
    }
    if (t == 0) h.hist_loss[r] = sum;
    if (h.keep_best && sum < cur) {  // workgroup-uniform
        for (int i = t; i < (d.Pimg >> 2); i += T)
            reinterpret_cast<float4*>(h.best_image)[i] = reinterpret_cast<const float4*>(image)[i];
        if (t == 0) {
            h.best[0] = sum;
            h.best[1] = __int_as_float(r);
        }
    }
}

static inline size_t ho_lds_bytes(const MLPDesc& d) { return (size_t)d.lds_floats * sizeof(float); }

hipError_t fl_set_lds_limit_heldout(size_t bytes) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fl_heldout_rows_kernel<1>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(fl_heldout_rows_kernel<2>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e;
}

static bool ho_shape_ok(const MLPDesc& d, int R, int n) {
    return (R == 16 || R == 32) && n >= 1 && n <= FL_HELDOUT_MAX_ROWS && d.L >= 1 && d.L <= FL_MAX_LAYERS &&
           d.dim[d.L] >= 1 && d.dim[d.L] <= FL_MAX_CLASSES && (d.Pimg & 3) == 0 &&
           ho_lds_bytes(d) + FL_HO_STATIC_INTS * sizeof(int) <= (size_t)160 * 1024;
}

template <int RT>
static void ho_launch_rows(const MLPDesc& d, const FLHeldout& p, const float* params, const FLState* st, float* proba,
                           int* pred, hipStream_t s) {
    hipLaunchKernelGGL(fl_heldout_rows_kernel<RT>, dim3((p.n + RT * 16 - 1) / (RT * 16)), dim3(FL_THREADS),
                       ho_lds_bytes(d), s, d, p, params, st, proba, pred);
}

hipError_t fl_launch_heldout(const MLPDesc& d, int R, const FLHeldout& p, const float* image, const FLState* st,
                             hipStream_t s) {
    if (!ho_shape_ok(d, R, p.n) || p.X == nullptr || p.y == nullptr || p.scratch == nullptr || p.hist_cm == nullptr ||
        p.hist_loss == nullptr || p.max_rounds < 1 || image == nullptr || st == nullptr ||
        (p.keep_best && (p.best_image == nullptr || p.best == nullptr || p.best_image == image)))
        return hipErrorInvalidValue;
    if (R == 16) ho_launch_rows<1>(d, p, image, st, nullptr, nullptr, s);
    else ho_launch_rows<2>(d, p, image, st, nullptr, nullptr, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fl_heldout_fold_kernel, dim3(1), dim3(FL_HELDOUT_FOLD_THREADS), 0, s, d, p, (p.n + R - 1) / R,
                       image, st);
    return hipGetLastError();
}

hipError_t fl_launch_heldout_predict(const MLPDesc& d, int R, const float* X, int n, const float* params, float* proba,
                                     int* pred, hipStream_t s) {
    if (!ho_shape_ok(d, R, n) || X == nullptr || params == nullptr || (proba == nullptr && pred == nullptr))
        return hipErrorInvalidValue;
    FLHeldout p = {};
    p.X = X;
    p.n = n;
    if (R == 16) ho_launch_rows<1>(d, p, params, nullptr, proba, pred, s);
    else ho_launch_rows<2>(d, p, params, nullptr, proba, pred, s);
    return hipGetLastError();
}
