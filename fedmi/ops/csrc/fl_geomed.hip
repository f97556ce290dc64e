// Geometric-median aggregation of a FedAvg round (Pillutla, Kakade, Harchaoui 2022, "Robust Aggregation
// for Federated Learning", RFA): after the K clients published their contributions (the unscaled
// post-step local models, as for fl_robust), T smoothed Weiszfeld iterations from the coordinate-wise
// median replace the weighted sum.  With S the round's sampled clients (rtab mask of the round in `st`,
// ANDed with the kept word of a screen, fl_screen.hip, when there is one), v_i client i's image,
// nu = FLGeomed::nu:
//
//   z_0 = the coordinate-wise median of S (fl_robust_select.h: the bits of fl_robust's median)
//   for t = 0 .. T - 1:
//     d_i  = sum over the real parameters p of the image of (v_i[p] - z_t[p])^2,  i in S
//     incl = { i in S : d_i < +inf }                 (NaN, inf, overflow: out for this iteration)
//     b_i  = 1 / max(nu, sqrt(d_i))                  (sqrtf: correctly rounded; __fdiv_rn)
//     B    = sum of b_i over incl, client order from +0
//     z_{t+1}[p] = (sum over incl, client order from +0, of b_i * v_i[p]) / B;   incl empty: z_{t+1} = z_t
//   result = z_T
//
// Every operation is one round-to-nearest fp32 operation (__fsub_rn, __fadd_rn, __fdiv_rn; the products
// by geomed_mul below, which no flag contracts into the sum they feed) and every sum has ONE order, so
// the result is bit-identical on every rank and across replays; fedmi/fl/aggregate.py geomed_model is
// the host model of it, bit for bit.  Excluded clients
// are selected out, never multiplied by 0: their images may hold NaN.  The aggregate is unweighted, as
// the median's is.
//
// The summation order of d_i.  The image is cut into blocks of FL_GEOMED_THREADS = 256 consecutive
// floats, block w = floats [256 w, 256 w + 256); position p of a block contributes (v_i[p] - z[p])^2, or
// +0 when p is image padding (fl_image_lim) or lies past the image.  A block's 256 terms are added as
// block_sum_ordered adds them: the xor tree (offsets 32, 16, ... 1) over each run of 64, then the four
// sums in order from +0.  d_i is the left fold, from +0, of the block sums in block order.  The order
// depends on the image alone -- not on K, its bucket or the launch.
//
// Launches: T + 1, the fused shape.  The combine of iteration t + 1 needs the K weights only, not z_t,
// and a thread that has just produced z[p] still holds the K values v_i[p].  So one workgroup per block,
// one owner thread per float, and launch `it` (0 .. T):
//   1. (it > 0) wave 0, lane i = client i, folds launch it - 1's per-block partials in block order into
//      d_i, takes b_i and the ballot of incl; an empty incl takes the weights the previous launch
//      combined with instead (its record in the scratch; none: the median), so z_t is produced again
//      bit for bit without ever having been stored;
//   2. estimates z[p]: the median (it = 0, or no iteration has combined yet) or the weighted combine;
//   3. (it < T) stores its block's K partial sums of (v_i - z)^2 for the next launch; (it = T) writes z
//      to all n_dst destinations, image padding exact 0 whatever the sources hold, and the metric tails
//      -- the left fold over all K sources in source order -- in workgroups of their own.
// No intermediate z is written.  The two sets of partials alternate (launch `it` reads set (it - 1) & 1
// and writes set it & 1); workgroup 0 stores iteration it - 1's record (FL_GEOMED_SLOT floats: weights,
// distances, combined mask) where tests and the next launch find it.  The destinations may be the
// sources: nothing is written before the last launch, and there a float has one owner that reads all K
// sources before it writes.  A round that is not live (fl_round_gate), or whose mask is empty, is the
// whole-buffer left fold in the last launch and touches no scratch.  No launch takes a per-round host
// argument.  No atomics, no grid barrier, LDS for the wave sums and the K weights only, plain vector
// stores.  Instantiated per K bucket 4 / 8 / 16 / 32 / 64 with every loop unrolled, as fl_robust is;
// slots past K re-read source K - 1 and are masked out.
#include "fl_common.h"
#include "fl_device.h"
#include "fl_image.h"
#include "fl_robust_select.h"

// The combine is a product that feeds a sum.  __fmul_rn / __fadd_rn are the plain operators unless the
// rounded OCML operations are enabled, and the compiler may then contract the pair into one fma -- one
// rounding where the rule has two.  These two are compiled with contraction off, so they stay a
// v_mul_f32 and a v_add_f32 whatever the flags (and so does the rest of this file).
#pragma clang fp contract(off)
__device__ __forceinline__ float geomed_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float geomed_add(float a, float b) { return a + b; }

template <int KB>
__global__ void __launch_bounds__(FL_GEOMED_THREADS)
fl_geomed_kernel(MLPDesc d, FLGeomed p, const float* const* __restrict__ src, float* const* __restrict__ dst, int n_dst,
                 const FLState* __restrict__ st, int tails_len, int img_blocks, float* scratch, int it,
                 const unsigned long long* __restrict__ keep) {
    __shared__ float sb[FL_GEOMED_MAX_K];
    __shared__ unsigned long long sincl;
    __shared__ float wsum[KB][FL_GEOMED_THREADS / 64];
    const bool last = it == p.T;
    if ((int)blockIdx.x >= img_blocks) {
        // metric tails (last launch only): one float per thread
        const int j = ((int)blockIdx.x - img_blocks) * FL_GEOMED_THREADS + threadIdx.x;
        if (j >= tails_len) return;
        const float out = fl_src_fold<KB, KB>(src, p.K, d.Pimg + j);  // (K <= KB, the launcher's bucket)
        for (int q = 0; q < n_dst; ++q) dst[q][d.Pimg + j] = out;
        return;
    }
    int r;
    uint64_t mask = fl_round_gate(st, p.max_rounds, r) ? fl_round_mask(p.rtab, r, p.K) : 0;
    if (keep != nullptr && mask != 0) mask &= *keep;
    const int idx = blockIdx.x * FL_GEOMED_THREADS + threadIdx.x;
    const bool in = idx < d.Pimg;
    const int li = in ? idx : d.Pimg - 1;   // (threads past the image stay for the block sums and add +0)
    if (mask == 0 && !last) return;         // (uniform) not live: only the last launch acts
    float v[KB][1];
    fl_src_load<KB, 1>(src, p.K, 0, li, v);
    if (mask == 0) {
        if (!in) return;
        const float out = fl_fold_loaded<KB, 1>(v, p.K, 0, 0, 0.f);
        for (int q = 0; q < n_dst; ++q) dst[q][idx] = out;
        return;
    }

    // 1. the weights of this launch's combine, from the previous launch's partials
    uint64_t incl = 0;
    if (it > 0) {
        if (threadIdx.x < 64) {
            const int i = threadIdx.x;
            const bool mine = ((mask >> i) & 1) != 0;   // (bits >= K are cut by fl_round_mask)
            const float* pin = scratch + (size_t)((it - 1) & 1) * img_blocks * FL_GEOMED_MAX_K + i;
            float di = 0.f;
            if (mine) {
#pragma unroll 8
                for (int w = 0; w < img_blocks; ++w) di = __fadd_rn(di, pin[(size_t)w * FL_GEOMED_MAX_K]);
            }
            const float inf = __uint_as_float(0x7f800000u);
            const bool ok = mine && di < inf;
            float bi = ok ? __fdiv_rn(1.f, fmaxf(p.nu, sqrtf(di))) : 0.f;
            uint64_t m = __ballot(ok);
            float* slots = scratch + 2 * (size_t)img_blocks * FL_GEOMED_MAX_K;
            if (m == 0 && it > 1) {
                // nobody is at a finite distance: z stays what the previous launch made it
                const float* prev = slots + (size_t)(it - 2) * FL_GEOMED_SLOT;
                const uint32_t* pm = reinterpret_cast<const uint32_t*>(prev + 2 * FL_GEOMED_MAX_K);
                m = ((uint64_t)pm[1] << 32) | pm[0];
                bi = prev[i];
            }
            sb[i] = bi;
            if (i == 0) sincl = m;
            if (blockIdx.x == 0) {
                float* slot = slots + (size_t)(it - 1) * FL_GEOMED_SLOT;
                slot[i] = bi;
                slot[FL_GEOMED_MAX_K + i] = mine ? (ok ? di : inf) : 0.f;
                if (i < 2) reinterpret_cast<uint32_t*>(slot + 2 * FL_GEOMED_MAX_K)[i] = (uint32_t)(m >> (32 * i));
            }
        }
        __syncthreads();
        incl = sincl;
    }

    // 2. the estimate at this thread's float
    float z;
    if (incl == 0) {   // (uniform)
        const int kr = __popcll(mask);
        const int t = (kr - 1) / 2;
        z = robust_select<KB, 1>(v, 0, mask, t, kr - t, (float)(kr - 2 * t));
    } else {
        float acc = 0.f, B = 0.f;
#pragma unroll
        for (int i = 0; i < KB; ++i) {
            const float bi = sb[i];
            const bool on = ((incl >> i) & 1) != 0;
            acc = on ? geomed_add(acc, geomed_mul(bi, v[i][0])) : acc;
            B = on ? __fadd_rn(B, bi) : B;
        }
        z = __fdiv_rn(acc, B);
    }
    const bool real = in && (idx & 3) < fl_image_lim(d, idx & ~3);

    if (last) {
        if (!in) return;
        const float out = real ? z : 0.f;
        for (int q = 0; q < n_dst; ++q) dst[q][idx] = out;
        return;
    }

    // 3. this block's partial sums of the squared distances to z, client by client
#pragma unroll
    for (int i = 0; i < KB; ++i) {
        if (!((mask >> i) & 1)) continue;   // (uniform)
        const float df = __fsub_rn(v[i][0], z);
        const float sq = wave_sum(real ? geomed_mul(df, df) : 0.f);
        if ((threadIdx.x & 63) == 0) wsum[i][threadIdx.x >> 6] = sq;
    }
    __syncthreads();
    if (threadIdx.x < FL_GEOMED_MAX_K) {
        const int i = threadIdx.x;
        float ss = 0.f;
        if (i < KB && ((mask >> i) & 1)) {
#pragma unroll
            for (int k = 0; k < FL_GEOMED_THREADS / 64; ++k) ss = __fadd_rn(ss, wsum[i][k]);
        }
        scratch[((size_t)(it & 1) * img_blocks + blockIdx.x) * FL_GEOMED_MAX_K + i] = ss;
    }
}

template <int KB>
static void geomed_launch(const MLPDesc& d, const FLGeomed& p, const float* const* src, float* const* dst, int n_dst,
                          const FLState* st, int tails_len, float* scratch, hipStream_t s,
                          const unsigned long long* keep) {
    const int img_blocks = fl_geomed_blocks(d.Pimg);
    const int tail_blocks = (tails_len + FL_GEOMED_THREADS - 1) / FL_GEOMED_THREADS;
    for (int it = 0; it <= p.T; ++it)
        hipLaunchKernelGGL((fl_geomed_kernel<KB>), dim3(img_blocks + (it == p.T ? tail_blocks : 0)),
                           dim3(FL_GEOMED_THREADS), 0, s, d, p, src, dst, n_dst, st, tails_len, img_blocks, scratch, it,
                           keep);
}

hipError_t fl_launch_geomed(const MLPDesc& d, const FLGeomed& p, const float* const* src, float* const* dst, int n_dst,
                            const FLState* st, int tails_len, float* scratch, hipStream_t s,
                            const unsigned long long* keep) {
    if ((d.Pimg & 3) != 0 || d.Pimg < 4 || src == nullptr || dst == nullptr || st == nullptr || scratch == nullptr ||
        p.rtab == nullptr || p.K < 1 || p.K > FL_GEOMED_MAX_K || n_dst < 1 || tails_len < 0 || p.max_rounds < 1 ||
        p.T < 1 || p.T > FL_GEOMED_MAX_ITERS || !(p.nu > 0.f) || !(p.nu < __builtin_huge_valf()))
        return hipErrorInvalidValue;
    if (p.K <= 4) geomed_launch<4>(d, p, src, dst, n_dst, st, tails_len, scratch, s, keep);
    else if (p.K <= 8) geomed_launch<8>(d, p, src, dst, n_dst, st, tails_len, scratch, s, keep);
    else if (p.K <= 16) geomed_launch<16>(d, p, src, dst, n_dst, st, tails_len, scratch, s, keep);
    else if (p.K <= 32) geomed_launch<32>(d, p, src, dst, n_dst, st, tails_len, scratch, s, keep);
    else geomed_launch<64>(d, p, src, dst, n_dst, st, tails_len, scratch, s, keep);
    return hipGetLastError();
}
