// The per-coordinate rule of the robust aggregators (fl_robust.hip: coordinate-wise median / trimmed
// mean, Yin et al. 2018), shared by the kernel over K local buffers (fl_robust.hip) and the one-shot
// xGMI gather-select kernel (peer_allreduce.hip), so both produce the same bits: the sortable key
// of a float and the rank-by-counting selection with its client-order sum.
#pragma once
#include "fl_common.h"
#include "fl_image.h"

// Sortable image of a float: unsigned order of the keys = the total order "any NaN above +inf,
// otherwise by value, -0 and +0 tie".
__device__ __forceinline__ uint32_t robust_key(float x) {
    const uint32_t u = __float_as_uint(x);
    const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return (u & 0x7fffffffu) > 0x7f800000u ? 0xfffffffeu : (u == 0x80000000u ? 0x80000000u : k);
}

// Median / trimmed mean of column e: ranks in [lo, hi) are kept, n = float(hi - lo).
template <int KB, int VEC>
__device__ __forceinline__ float robust_select(const float (&v)[KB][VEC], int e, uint64_t mask, int lo, int hi,
                                               float n) {
    uint32_t key[KB];
    int rank[KB];
#pragma unroll
    for (int i = 0; i < KB; ++i) {
        key[i] = ((mask >> i) & 1) ? robust_key(v[i][e]) : 0xffffffffu;
        rank[i] = 0;
    }
#pragma unroll
    for (int i = 1; i < KB; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) {
            const int before = key[j] <= key[i] ? 1 : 0;  // j < i: j sorts before i on a tie
            rank[i] += before;
            rank[j] += 1 - before;
        }
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < KB; ++i) acc = (rank[i] >= lo && rank[i] < hi) ? __fadd_rn(acc, v[i][e]) : acc;
    return __fdiv_rn(acc, n);
}

// The whole rule for the VEC loaded values of K <= KB sources at image float `idx`: the round's sampled
// clients `mask` (0: the round is not live -- the left fold in source order, padding included);
// image padding exact 0 (fl_image.h fl_image_lim).
template <int KB, int VEC>
__device__ __forceinline__ void robust_apply(const MLPDesc& d, const FLRobust& p, const float (&v)[KB][VEC], int K,
                                             int idx, uint64_t mask, float (&out)[VEC]) {
    const int kr = __popcll(mask);
    if (kr == 0) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) out[e] = fl_fold_loaded<KB, VEC>(v, K, 0, e, 0.f);
        return;
    }
    const int t = fl_robust_trim(p.kind, p.beta, kr);
    const float n = (float)(kr - 2 * t);
    const int lim = fl_image_lim(d, idx & ~3) - (idx & 3);  // elements e < lim are real parameters
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const float a = robust_select<KB, VEC>(v, e, mask, t, kr - t, n);
        out[e] = e < lim ? a : 0.f;
    }
}
