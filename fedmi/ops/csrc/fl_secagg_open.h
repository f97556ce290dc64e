// The per-coordinate open of secure aggregation (fl_secagg.hip; Bonawitz et al. 2017, the arithmetic
// only), shared by the kernel over K local buffers (fl_secagg.hip) and the one-shot xGMI gather-select
// kernel (peer_allreduce.hip), so both produce the same bits: the uint32 sum mod 2^32 of the sampled
// sources' words with the fp32 left fold of all sources beside it, and the scaling of the sum.
#pragma once
#include "fl_common.h"
#include "fl_image.h"

// 2^bits and 2^-bits of the launch (powers of two: exact); false: bits out of range.
static inline bool fl_secagg_scales(FLSecAgg& p) {
    if (p.bits < FL_SECAGG_MIN_BITS || p.bits > FL_SECAGG_MAX_BITS) return false;
    p.scale = (float)(1u << p.bits);
    p.inv_scale = 1.f / p.scale;
    return true;
}

// Source `i` of K (`in`: i < K; `on`: it is one of the round's sampled clients) into the running integer
// sum of the words' bit patterns and, beside it, the left fold in source order of a round that is not live.
__device__ __forceinline__ void sa_open_add(uint32_t (&S)[4], float (&acc)[4], const float (&v)[4], int i, bool in,
                                            bool on) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        S[e] += on ? __float_as_uint(v[e]) : 0u;
        acc[e] = i == 0 ? v[e] : (in ? __fadd_rn(acc[e], v[e]) : acc[e]);
    }
}

// The opened float4 at image float `idx` (a multiple of 4): float(int32(S)) * 2^-F on the real parameters,
// padding exact 0; a round that is not live (mask == 0): the fold, padding included.
__device__ __forceinline__ void sa_open_finish(const MLPDesc& d, int idx, uint64_t mask, const uint32_t (&S)[4],
                                               const float (&acc)[4], float inv_scale, float (&out)[4]) {
    if (mask == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = acc[e];
        return;
    }
    const int lim = fl_image_lim(d, idx);  // elements e < lim are real parameters
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = e < lim ? __fmul_rn((float)(int)S[e], inv_scale) : 0.f;
}
