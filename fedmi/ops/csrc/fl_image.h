// What the kernels that run after the Adam kernel (fl_dp, fl_compress, fl_server, fl_robust,
// fl_secagg) share: how the padded parameter image (fl_common.h) is addressed, the gate that makes
// a round past a stop an exact no-op with the accessors of the round's rtab row, and the K-source
// loads and left fold of the aggregators.  One statement of each rule; fl_adam_map.h holds the
// Adam kernels' own copy of the index rule (with the packed bf16 position beside it), and
// tests/native/test_image_index.cpp ties the two together.
#pragma once
#include "fl_common.h"

// Dense (named_parameters() order) index -> image position, as the Adam kernel maps it
// (fl_adam_map.h, run-time arm): the layer's offsets by compile-time-indexed selects, row stride
// fl_ldw(K), chunk swizzle fl_swz(n), biases behind the weights.
__host__ __device__ __forceinline__ constexpr int fl_image_index(const MLPDesc& d, int di) {
    int K = d.dim[0], wo = d.w_off[0], bo = d.b_off[0], iwo = d.iw_off[0], ibo = d.ib_off[0];
#pragma unroll
    for (int t = 1; t < FL_MAX_LAYERS; ++t)
        if (t < d.L && di >= d.w_off[t]) {
            K = d.dim[t]; wo = d.w_off[t]; bo = d.b_off[t]; iwo = d.iw_off[t]; ibo = d.ib_off[t];
        }
    if (di >= bo) return ibo + (di - bo);
    const int q = di - wo;
    const int n = q / K, k = q - n * K;
    return iwo + n * fl_ldw(K) + (k ^ fl_swz(n));
}

// The inverse question.  Real parameters of the image's float4 that starts at float `idx` (a
// multiple of 4): its elements j < fl_image_lim are parameters, the rest image padding (rows >= N,
// columns >= K, the 4 pad floats of a row, bias slots >= N); <= 0: all padding.  The layer by
// compile-time-indexed selects; a float4 lies in one row and one 4-float swizzle chunk (fl_ldw and
// the chunk swizzle are multiples of 4).
__host__ __device__ inline int fl_image_lim(const MLPDesc& d, int idx) {
    int K = d.dim[0], N = d.dim[1], iwo = d.iw_off[0], ibo = d.ib_off[0];
#pragma unroll
    for (int t = 1; t < FL_MAX_LAYERS; ++t)
        if (t < d.L && idx >= d.iw_off[t]) {
            K = d.dim[t]; N = d.dim[t + 1]; iwo = d.iw_off[t]; ibo = d.ib_off[t];
        }
    if (idx >= ibo) return N - (idx - ibo);
    const int ldw = fl_ldw(K);
    const int q = idx - iwo;
    const int n = q / ldw, c = q - n * ldw;
    return n < N ? K - (c ^ fl_swz(n)) : 0;
}

// The round gate: true, with `r` the round's index, when the launch's round is live (not past an
// early stop) and inside [0, max_rounds).  `r` is not written otherwise: cur_round is valid only
// when live.
__device__ __forceinline__ bool fl_round_gate(const FLState* __restrict__ st, int max_rounds, int& r) {
    if (!st->live) return false;
    r = st->cur_round;
    return r >= 0 && r < max_rounds;
}

// Row r of the per-round table (FLBuffers::rtab): this client's FedAvg weight (0: not sampled), and
// the 64-bit mask of the round's sampled clients, optionally cut to clients 0 .. K - 1.  (The
// Adam / train kernels' metric fold, fl_device.h fold_round, reads the same row in place.)
__device__ __forceinline__ float fl_round_weight(const float* rtab, int r) { return rtab[4 * (size_t)r]; }
__device__ __forceinline__ uint64_t fl_round_mask(const float* rtab, int r, int K = 64) {
    const uint32_t* rt = reinterpret_cast<const uint32_t*>(rtab) + 4 * (size_t)r;
    const uint64_t mask = ((uint64_t)rt[3] << 32) | rt[2];
    return K < 64 ? mask & ((1ull << K) - 1ull) : mask;
}

// Sources [i0, i0 + B) of a float / float4 at float `idx`: all loads issued, nothing used; slots
// past K re-read source K - 1.
template <int B, int VEC>
__device__ __forceinline__ void fl_src_load(const float* const* __restrict__ src, int K, int i0, int idx,
                                            float (&v)[B][VEC]) {
#pragma unroll
    for (int i = 0; i < B; ++i) {
        const float* s = src[i0 + i < K ? i0 + i : K - 1];
        if constexpr (VEC == 4) {
            const float4 x = *reinterpret_cast<const float4*>(s + idx);
            v[i][0] = x.x; v[i][1] = x.y; v[i][2] = x.z; v[i][3] = x.w;
        } else {
            v[i][0] = s[idx];
        }
    }
}

// Left fold in source order, as the one-shot all-reduce sums: column e of the loaded sources
// [i0, i0 + B) folded into `acc` (source 0 starts it; slots past K are skipped).
template <int B, int VEC>
__device__ __forceinline__ float fl_fold_loaded(const float (&v)[B][VEC], int K, int i0, int e, float acc) {
#pragma unroll
    for (int i = 0; i < B; ++i) acc = i0 + i == 0 ? v[i][e] : (i0 + i < K ? __fadd_rn(acc, v[i][e]) : acc);
    return acc;
}

// The metric tails behind the image (every client fills its own slot): that fold of float `idx`
// over all K sources (1 <= K <= KMAX, the launcher's bound), the loads of B sources in flight per
// trip; KMAX == B is one trip and compiles without a loop.
template <int B, int KMAX>
__device__ __forceinline__ float fl_src_fold(const float* const* __restrict__ src, int K, int idx) {
    float acc = 0.f;
    for (int i0 = 0; i0 < (B == KMAX ? 1 : K); i0 += B) {
        float v[B][1];
        fl_src_load<B, 1>(src, K, i0, idx, v);
        acc = fl_fold_loaded<B, 1>(v, K, i0, 0, acc);
    }
    return acc;
}
