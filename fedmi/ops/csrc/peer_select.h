// Data phase of the one-shot xGMI gather-select kernel (peer_allreduce.hip peer_select_kernel): where
// the all-reduce sums the ranks' float4s (peer_device.h peer_reduce4), this selects -- the robust
// aggregators' coordinate-wise median / trimmed mean (fl_robust_select.h) -- or opens -- secure
// aggregation's integer sum of the masked words (fl_secagg_open.h) -- the very rules of the kernels
// over local buffers (fl_robust.hip, fl_secagg.hip), so both planes produce the same bits.  Source j is
// rank j = client j; the round's sampled clients come from the rtab row of the round in `st`.
#pragma once
#include "fl_image.h"
#include "fl_robust_select.h"
#include "fl_secagg_open.h"
#include "peer_device.h"

#define PEER_SELECT_ROBUST 1
#define PEER_SELECT_OPEN 2

// Parameters of a select call (the rule of `mode` alone is read).
struct PeerSelect {
    int mode;        // PEER_SELECT_*
    MLPDesc d;       // the parameter image: the call's first d.Pimg floats
    FLRobust rb;     // K = world
    FLSecAgg sa;     // K = world, inv_scale filled in
};

// out[4 i] for the float4s i of the image (block `bid` of `nb` takes a grid-stride share): all `world`
// loads issued before the first use (slots past `world` hold zeros and are masked out / not folded),
// then the rule; optional bf16 pack of the result.
template <int MODE, int KB>
__device__ __forceinline__ void peer_select4(const PeerArgs& a, const PeerPack& pk, const PeerSelect& p,
                                             const FLState* __restrict__ st, int bid, int nb) {
    const int bytes = (int)(a.n * 4);
    const long long i1 = p.d.Pimg >> 2;
    // the round's sampled ranks (0: not live)
    int r;
    const int max_rounds = MODE == PEER_SELECT_ROBUST ? p.rb.max_rounds : p.sa.max_rounds;
    const float* rtab = MODE == PEER_SELECT_ROBUST ? p.rb.rtab : p.sa.rtab;
    const uint64_t mask = fl_round_gate(st, max_rounds, r) ? fl_round_mask(rtab, r, a.world) : 0;
    for (long long i = (long long)bid * blockDim.x + threadIdx.x; i < i1; i += (long long)nb * blockDim.x) {
        float v[KB][4];
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            // (bit patterns: nothing but moves between the load and the rule)
            const float4 x = j < a.world ? peer_load16(a.src[j], bytes, (int)(i * 16)) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[j][0] = x.x; v[j][1] = x.y; v[j][2] = x.z; v[j][3] = x.w;
        }
        float out[4];
        if constexpr (MODE == PEER_SELECT_ROBUST) {
            robust_apply<KB, 4>(p.d, p.rb, v, a.world, (int)(4 * i), mask, out);
        } else {
            uint32_t S[4] = {0u, 0u, 0u, 0u};
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < KB; ++j) sa_open_add(S, acc, v[j], j, j < a.world, j < a.world && ((mask >> j) & 1));
            sa_open_finish(p.d, (int)(4 * i), mask, S, acc, p.sa.inv_scale, out);
        }
        const float4 s = make_float4(out[0], out[1], out[2], out[3]);
        reinterpret_cast<float4*>(a.out)[i] = s;
        if (pk.pk != nullptr) peer_pack_store(pk, (int)i, s);
    }
}
