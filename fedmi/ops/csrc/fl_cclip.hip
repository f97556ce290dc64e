// Centered-clipping aggregation of a FedAvg round (Karimireddy, He, Jaggi 2021, "Learning from History for
// Byzantine Robust Optimization"): after the K clients published their contributions (the unscaled post-step
// local models, as for fl_robust), T clipping iterations from the image the round trained from replace the
// weighted sum.  With S the round's sampled clients (rtab mask of the round in `st`, ANDed with the kept word
// of a screen, fl_screen.hip, when there is one), K_r = |S|, v_i client i's image, x the round's input image,
// tau = FLCclip::tau:
//
//   z_0 = x
//   for l = 0 .. T - 1:
//     d_i  = sum over the real parameters p of the image of (v_i[p] - z_l[p])^2,  i in S
//     ok   = { i in S : d_i < +inf }                 (NaN, inf, overflow: out for this iteration)
//     c_i  = sqrt(d_i) > tau ? tau / sqrt(d_i) : 1   (sqrtf: correctly rounded; __fdiv_rn)
//     g[p] = sum over ok, client order from +0, of c_i * (v_i[p] - z_l[p])
//     z_{l+1}[p] = z_l[p] + g[p] / K_r;   ok empty: z_{l+1} = z_l (selected, not added)
//   result = z_T
//
// The divisor is K_r, not |ok|: an excluded client pulls with zero force and gains nothing by it.  Every
// operation is one round-to-nearest fp32 operation (the file is compiled with contraction off, see below)
// and every sum has ONE order, so the result is bit-identical on every rank and across replays;
// fedmi/fl/aggregate.py cclip_model is the host model of it, bit for bit.  Excluded clients are selected out,
// never multiplied by 0: their images may hold NaN.  The aggregate is unweighted, as the median's is.
//
// The summation order of d_i is fl_geomed.hip's, unchanged: blocks of FL_CCLIP_THREADS = 256 consecutive
// floats, position p contributing (v_i[p] - z[p])^2 or +0 when p is image padding (fl_image_lim) or lies past
// the image; a block's 256 terms added as block_sum_ordered adds them (the xor tree over each run of 64, the
// four sums in order from +0); d_i the left fold, from +0, of the block sums in block order.
//
// Launches: T + 1, and no z_l is ever written.  Unlike Weiszfeld's combine the recursion needs z_l itself --
// but z_l[p] is a function of x[p], the K values v_i[p] and the l records (c, ok) of the iterations before
// it, K + 1 registers and l x 65 words that every thread can hold.  So one workgroup per block, one owner
// thread per float, x[p] and the K values loaded once (all loads in flight before the first use) and kept
// in registers, and launch `it` (0 .. T):
//   1. (it > 0) the block's first wave, lane i = client i, reads the records of iterations 0 .. it - 2 from
//      the scratch into LDS (workgroup 0 of the launches before stored them);
//   2. (it > 0) the same lanes fold launch it - 1's per-block partials in block order into d_i, take c_i
//      and the ballot of ok: iteration it - 1's record, left in LDS beside the others;
//   3. (it > 0) workgroup 0 stores that record in the scratch, where tests and later launches find it;
//   4. every thread replays z_1 .. z_it at its float: it x K multiply-adds on registers and LDS broadcasts,
//      the same operations in every launch and so the same bits -- z_l is produced again, not read back;
//   5. (it < T) stores its block's K partial sums of (v_i - z_it)^2 into partial set it & 1 (the next
//      launch reads that set while it writes the other);
//   6. (it = T) writes z_T to all n_dst destinations, image padding exact 0 whatever the sources hold, and
//      the metric tails -- the left fold over all K sources in source order -- in workgroups of their own.
// A stored z would cost a Pimg write and read per iteration and a buffer; the replay costs T (T + 1) / 2
// combines of K registers per float, which FL_CCLIP_MAX_ITERS = 8 bounds.  Nothing is written to a
// destination before the last launch, and there a float has one owner that reads x and all K sources before
// it writes, so the destinations may be the sources; x must not be a destination (the launcher refuses it).
// A round that is not live (fl_round_gate), or whose mask is empty, is the whole-buffer left fold in the last
// launch and touches no scratch.  No launch takes a per-round host argument.  No atomics, no grid barrier,
// LDS for the wave sums and the T x 64 clip factors (with their masks) only, plain vector stores.
// Instantiated per K bucket 4 / 8 / 16 / 32 / 64 with every K loop unrolled, as fl_robust is; slots past K
// re-read source K - 1 and are masked out.
#include "fl_common.h"
#include "fl_device.h"
#include "fl_image.h"

// The pull is a product that feeds a sum, the distance a product that feeds a tree of sums.  __fmul_rn /
// __fadd_rn are the plain operators unless the rounded OCML operations are enabled, and the compiler may then
// contract the pair into one fma -- one rounding where the rule has two (fl_geomed.hip and fl_attack.hip
// record that their first builds did).  These are compiled with contraction off, so they stay a v_mul_f32
// and a v_add_f32 whatever the flags (and so does the rest of this file).
#pragma clang fp contract(off)
__device__ __forceinline__ float cclip_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float cclip_add(float a, float b) { return a + b; }

template <int KB>
__global__ void __launch_bounds__(FL_CCLIP_THREADS)
fl_cclip_kernel(MLPDesc d, FLCclip p, const float* const* __restrict__ src, const float* __restrict__ x,
                float* const* __restrict__ dst, int n_dst, const FLState* __restrict__ st, int tails_len, int img_blocks,
                float* scratch, int it, const unsigned long long* __restrict__ keep) {
    __shared__ float sc[FL_CCLIP_MAX_ITERS][FL_CCLIP_MAX_K];   // clip factors of iterations 0 .. it - 1
    __shared__ unsigned long long sok[FL_CCLIP_MAX_ITERS];     // ... and their included masks
    __shared__ float wsum[KB][FL_CCLIP_THREADS / 64];
    const bool last = it == p.T;
    if ((int)blockIdx.x >= img_blocks) {
        // metric tails (last launch only): one float per thread
        const int j = ((int)blockIdx.x - img_blocks) * FL_CCLIP_THREADS + threadIdx.x;
        if (j >= tails_len) return;
        const float out = fl_src_fold<KB, KB>(src, p.K, d.Pimg + j);  // (K <= KB, the launcher's bucket)
        for (int q = 0; q < n_dst; ++q) dst[q][d.Pimg + j] = out;
        return;
    }
    int r;
    uint64_t mask = fl_round_gate(st, p.max_rounds, r) ? fl_round_mask(p.rtab, r, p.K) : 0;
    if (keep != nullptr && mask != 0) mask &= *keep;
    const int idx = blockIdx.x * FL_CCLIP_THREADS + threadIdx.x;
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
    float z = x[li];

    // 1. - 3. the records of iterations 0 .. it - 1: the earlier ones from the scratch, the newest from the
    // previous launch's partials
    if (it > 0) {
        if (threadIdx.x < 64) {
            const int i = threadIdx.x;
            float* slots = scratch + 2 * (size_t)img_blocks * FL_CCLIP_MAX_K;
            for (int l = 0; l + 1 < it; ++l) {
                const float* rec = slots + (size_t)l * FL_CCLIP_SLOT;
                sc[l][i] = rec[i];
                if (i == 0) {
                    const uint32_t* pm = reinterpret_cast<const uint32_t*>(rec + 2 * FL_CCLIP_MAX_K);
                    sok[l] = ((uint64_t)pm[1] << 32) | pm[0];
                }
            }
            const bool mine = ((mask >> i) & 1) != 0;   // (bits >= K are cut by fl_round_mask)
            const float* pin = scratch + (size_t)((it - 1) & 1) * img_blocks * FL_CCLIP_MAX_K + i;
            float di = 0.f;
            if (mine) {
#pragma unroll 8
                for (int w = 0; w < img_blocks; ++w) di = __fadd_rn(di, pin[(size_t)w * FL_CCLIP_MAX_K]);
            }
            const float inf = __uint_as_float(0x7f800000u);
            const bool ok = mine && di < inf;
            const float si = sqrtf(di);
            const float ci = ok ? (si > p.tau ? __fdiv_rn(p.tau, si) : 1.f) : 0.f;
            const uint64_t m = __ballot(ok);
            sc[it - 1][i] = ci;
            if (i == 0) sok[it - 1] = m;
            if (blockIdx.x == 0) {
                float* slot = slots + (size_t)(it - 1) * FL_CCLIP_SLOT;
                slot[i] = ci;
                slot[FL_CCLIP_MAX_K + i] = mine ? (ok ? di : inf) : 0.f;
                if (i < 2) reinterpret_cast<uint32_t*>(slot + 2 * FL_CCLIP_MAX_K)[i] = (uint32_t)(m >> (32 * i));
            }
        }
        __syncthreads();
    }

    // 4. the replay: z_1 .. z_it at this thread's float, from x, the K registers and the records in LDS
    const float kr = (float)__popcll(mask);
    for (int l = 0; l < it; ++l) {
        const uint64_t m = sok[l];   // (uniform)
        float g = 0.f;
#pragma unroll
        for (int i = 0; i < KB; ++i) {
            const bool on = ((m >> i) & 1) != 0;
            g = on ? cclip_add(g, cclip_mul(sc[l][i], __fsub_rn(v[i][0], z))) : g;
        }
        z = m != 0 ? cclip_add(z, __fdiv_rn(g, kr)) : z;
    }
    const bool real = in && (idx & 3) < fl_image_lim(d, idx & ~3);

    if (last) {
        if (!in) return;
        const float out = real ? z : 0.f;
        for (int q = 0; q < n_dst; ++q) dst[q][idx] = out;
        return;
    }

    // 5. this block's partial sums of the squared distances to z_it, client by client
#pragma unroll
    for (int i = 0; i < KB; ++i) {
        if (!((mask >> i) & 1)) continue;   // (uniform)
        const float df = __fsub_rn(v[i][0], z);
        const float sq = wave_sum(real ? cclip_mul(df, df) : 0.f);
        if ((threadIdx.x & 63) == 0) wsum[i][threadIdx.x >> 6] = sq;
    }
    __syncthreads();
    if (threadIdx.x < FL_CCLIP_MAX_K) {
        const int i = threadIdx.x;
        float ss = 0.f;
        if (i < KB && ((mask >> i) & 1)) {
#pragma unroll
            for (int k = 0; k < FL_CCLIP_THREADS / 64; ++k) ss = __fadd_rn(ss, wsum[i][k]);
        }
        scratch[((size_t)(it & 1) * img_blocks + blockIdx.x) * FL_CCLIP_MAX_K + i] = ss;
    }
}

template <int KB>
static void cclip_launch(const MLPDesc& d, const FLCclip& p, const float* const* src, const float* x, float* const* dst,
                         int n_dst, const FLState* st, int tails_len, float* scratch, hipStream_t s,
                         const unsigned long long* keep) {
    const int img_blocks = fl_cclip_blocks(d.Pimg);
    const int tail_blocks = (tails_len + FL_CCLIP_THREADS - 1) / FL_CCLIP_THREADS;
    for (int it = 0; it <= p.T; ++it)
        hipLaunchKernelGGL((fl_cclip_kernel<KB>), dim3(img_blocks + (it == p.T ? tail_blocks : 0)),
                           dim3(FL_CCLIP_THREADS), 0, s, d, p, src, x, dst, n_dst, st, tails_len, img_blocks, scratch, it,
                           keep);
}

hipError_t fl_launch_cclip(const MLPDesc& d, const FLCclip& p, const float* const* src, const float* x,
                           float* const* dst, int n_dst, const FLState* st, int tails_len, float* scratch,
                           hipStream_t s, const unsigned long long* keep, const unsigned long long* dst_host) {
    if ((d.Pimg & 3) != 0 || d.Pimg < 4 || src == nullptr || x == nullptr || dst == nullptr || st == nullptr ||
        scratch == nullptr || dst_host == nullptr || p.rtab == nullptr || p.K < 1 || p.K > FL_CCLIP_MAX_K || n_dst < 1 || tails_len < 0 ||
        p.max_rounds < 1 || p.T < 1 || p.T > FL_CCLIP_MAX_ITERS || !(p.tau > 0.f) || !(p.tau < __builtin_huge_valf()))
        return hipErrorInvalidValue;
    // x is read by every launch and must outlive the sequence as it is: never a destination
    const unsigned long long x0 = (unsigned long long)(uintptr_t)x, x1 = x0 + sizeof(float) * (unsigned long long)d.Pimg;
    const unsigned long long row = sizeof(float) * ((unsigned long long)d.Pimg + (unsigned long long)tails_len);
    for (int q = 0; q < n_dst; ++q)
        if (dst_host[q] < x1 && x0 < dst_host[q] + row) return hipErrorInvalidValue;
    if (p.K <= 4) cclip_launch<4>(d, p, src, x, dst, n_dst, st, tails_len, scratch, s, keep);
    else if (p.K <= 8) cclip_launch<8>(d, p, src, x, dst, n_dst, st, tails_len, scratch, s, keep);
    else if (p.K <= 16) cclip_launch<16>(d, p, src, x, dst, n_dst, st, tails_len, scratch, s, keep);
    else if (p.K <= 32) cclip_launch<32>(d, p, src, x, dst, n_dst, st, tails_len, scratch, s, keep);
    else cclip_launch<64>(d, p, src, x, dst, n_dst, st, tails_len, scratch, s, keep);
    return hipGetLastError();
}
