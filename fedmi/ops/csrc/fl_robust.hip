// Byzantine-robust aggregation of a FedAvg round (Yin et al. 2018, "Byzantine-Robust Distributed
// Learning: Towards Optimal Statistical Rates"): one launch per round, after the K clients published
// their contributions (the unscaled post-step local models: the engine's FedAvg scale is 1 for a
// sampled client in robust mode), replaces the weighted sum by the coordinate-wise median or
// beta-trimmed mean.  With S_r the round's sampled clients (rtab mask of the round in `st`),
// K_r = |S_r| and t = fl_robust_trim (median (K_r - 1) / 2, trimmed mean floor(beta K_r)), per
// coordinate of the parameter image:
//
//   order the K_r values: any NaN above +inf, otherwise by value; ties (-0 and +0 tie) by client index
//   drop the t lowest and the t highest
//   acc = 0; acc = add(acc, v_k) over the kept clients in client order; result = div(acc, float(K_r - 2 t))
//
// Every operation is an explicit round-to-nearest fp32 intrinsic, so the result is bit-identical on
// every rank and across replays whatever the compile flags (as in fl_server.hip);
// fedmi/fl/aggregate.py robust_aggregate_torch is the host model of it.  The aggregate is
// unweighted: sample sizes are self-reported, and a weighted median is not what the paper analyses.
//
// Selection is rank by counting on the sortable-integer image of the float (NaN canonicalised to
// one key above +inf's, an unsampled slot to the key above that, so it ranks behind every sampled
// one): rank_i = #{j : key_j < key_i, or key_j == key_i and j < i}, each pair compared once.  That is
// K (K - 1) / 2 compares per coordinate, branch-free, no LDS, no atomics, no grid barrier.  The
// kernel is instantiated for K buckets 4 / 8 / 16 / 32 / 64 with every loop unrolled, so values,
// keys and ranks stay in registers (3 K per coordinate; a runtime-indexed array would live in
// scratch).  Buckets up to 8 take one float4 of the image per thread, the wider ones one float
// (float4 at 64 would need 768 registers).  Slots past K re-read source K - 1 and are masked out.
//
// One thread owns a coordinate: it reads it from all K sources -- every load issued before the
// first use, one L2 latency per thread -- and writes the result to all n_dst destinations, which may
// be sources (in place: nobody else reads or writes that coordinate).  Image padding of every
// destination is written as exact 0 whatever the sources hold: a tampered peer cannot break the
// zero-padding invariant the unpredicated MFMA operand reads rely on (fl_common.h).
//
// The metric tails behind the image (tails_len floats; every client fills its own slot) are the
// left fold over all K sources in source order, as the one-shot all-reduce sums them.  A round
// that is not live (past an early stop or past max_rounds; client 0 republished the global image,
// the others zeros) folds the whole buffer that way, padding included: it stays the exact no-op
// it is under the weighted sum.
//
// Behind a client screen (fl_screen.hip, multi-Krum) the launch gets the round's kept-client mask
// (`keep`, one device word; null without a screen): a live round ANDs it into the sampled mask, so the
// rule above runs over the kept clients and K_r is their number.  The tails and a round that is not
// live never read it.
//
// Launch- and latency-bound like fl_server: 64-thread workgroups, so the waves land on CUs of
// their own; the tails run in workgroups of their own (no wave mixes the two paths).  Plain vector
// stores only.
#include "fl_common.h"
#include "fl_image.h"
#include "fl_robust_select.h"

#define FL_ROBUST_THREADS 64

// (robust_key, robust_select and the whole per-coordinate rule robust_apply: fl_robust_select.h, shared with
// the one-shot xGMI gather-select kernel of peer_allreduce.hip)

template <int KB, int VEC>
__global__ void __launch_bounds__(FL_ROBUST_THREADS)
fl_robust_kernel(MLPDesc d, FLRobust p, const float* const* __restrict__ src, float* const* __restrict__ dst, int n_dst,
                 const FLState* __restrict__ st, int tails_len, int img_blocks,
                 const unsigned long long* __restrict__ keep) {
    if ((int)blockIdx.x >= img_blocks) {
        // metric tails: one float per thread
        const int j = ((int)blockIdx.x - img_blocks) * FL_ROBUST_THREADS + threadIdx.x;
        if (j >= tails_len) return;
        const float out = fl_src_fold<KB, KB>(src, p.K, d.Pimg + j);  // (K <= KB, the launcher's bucket)
        for (int q = 0; q < n_dst; ++q) dst[q][d.Pimg + j] = out;
        return;
    }
    const int u = blockIdx.x * FL_ROBUST_THREADS + threadIdx.x;
    const int idx = VEC * u;
    if (idx >= d.Pimg) return;
    float v[KB][VEC];
    fl_src_load<KB, VEC>(src, p.K, 0, idx, v);
    // the round's sampled clients, cut to the ones the round's screening kept (fl_screen.hip) if any
    int r;
    uint64_t mask = fl_round_gate(st, p.max_rounds, r) ? fl_round_mask(p.rtab, r, p.K) : 0;
    if (keep != nullptr && mask != 0) mask &= *keep;
    float out[VEC];
    robust_apply<KB, VEC>(d, p, v, p.K, idx, mask, out);
    for (int q = 0; q < n_dst; ++q) {
        float* o = dst[q] + idx;
        if constexpr (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(out[0], out[1], out[2], out[3]);
        else *o = out[0];
    }
}

template <int KB, int VEC>
static void robust_launch(const MLPDesc& d, const FLRobust& p, const float* const* src, float* const* dst, int n_dst,
                          const FLState* st, int tails_len, hipStream_t s, const unsigned long long* keep) {
    const int units = d.Pimg / VEC;
    const int img_blocks = (units + FL_ROBUST_THREADS - 1) / FL_ROBUST_THREADS;
    const int tail_blocks = (tails_len + FL_ROBUST_THREADS - 1) / FL_ROBUST_THREADS;
    hipLaunchKernelGGL((fl_robust_kernel<KB, VEC>), dim3(img_blocks + tail_blocks), dim3(FL_ROBUST_THREADS), 0, s, d, p,
                       src, dst, n_dst, st, tails_len, img_blocks, keep);
}

hipError_t fl_launch_robust(const MLPDesc& d, const FLRobust& p, const float* const* src, float* const* dst, int n_dst,
                            const FLState* st, int tails_len, hipStream_t s, const unsigned long long* keep) {
    if ((d.Pimg & 3) != 0 || d.Pimg < 4 || src == nullptr || dst == nullptr || st == nullptr || p.rtab == nullptr ||
        p.K < 1 || p.K > FL_ROBUST_MAX_K || n_dst < 1 || tails_len < 0 || p.max_rounds < 1 ||
        (p.kind != FL_ROBUST_MEDIAN && p.kind != FL_ROBUST_TRIMMED) || !(p.beta >= 0.0 && p.beta < 0.5))
        return hipErrorInvalidValue;
    if (p.K <= 4) robust_launch<4, 4>(d, p, src, dst, n_dst, st, tails_len, s, keep);
    else if (p.K <= 8) robust_launch<8, 4>(d, p, src, dst, n_dst, st, tails_len, s, keep);
    else if (p.K <= 16) robust_launch<16, 1>(d, p, src, dst, n_dst, st, tails_len, s, keep);
    else if (p.K <= 32) robust_launch<32, 1>(d, p, src, dst, n_dst, st, tails_len, s, keep);
    else robust_launch<64, 1>(d, p, src, dst, n_dst, st, tails_len, s, keep);
    return hipGetLastError();
}
