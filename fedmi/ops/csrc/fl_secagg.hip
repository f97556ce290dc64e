// Secure aggregation of a FedAvg round (Bonawitz et al. 2017, "Practical Secure Aggregation for
// Privacy-Preserving Machine Learning"), the protocol's ARITHMETIC only (one shared group seed, no
// key agreement, no dropout recovery, no malicious-server rounds): two launches per round, after the
// clients published their weighted fp32 contributions c_i (the Adam, DP or compression kernel's
// output).  With P_r the round's sampled clients (rtab mask of the round in `st`), K_r = |P_r|,
// F = FLSecAgg::bits, per dense parameter p:
//
//   fl_secagg_mask   L = (2^31 - 1) / K_r
//                    q_i = clamp(rint(c_i * 2^F), -L, L)        +-inf -> +-L, NaN -> 0, both counted
//                    y_i = q_i + sum_{j in P_r, j > i} m(i, j) - sum_{j in P_r, j < i} m(j, i)   mod 2^32
//                    m(a, b)[p] = word p % 4 of Philox4x32-10 at counter (p / 4, round, 64 a + b,
//                    FL_SECAGG_STREAM) under the group key; y_i's bit pattern replaces c_i in place
//   fl_secagg_open   S = sum_{i in P_r} y_i mod 2^32;  aggregate = float(int(S)) * 2^-F
//
// |q| <= L, so the true sum cannot wrap and the masks cancel exactly: the opened image does not
// depend on the key.  c * 2^F is exact in fp32 (or overflows to inf, which clamps; a flushed
// subnormal rounds to 0 either way), rint is half-to-even, the compare against L is an integer one;
// the open is one int-to-float rounding and an exact scaling.  fedmi/fl/secagg.py is the host model
// of both, bit for bit.
//
// Mask: one launch masks n buffers in place (blockIdx.y = buffer, client first_client + blockIdx.y).
// One thread per quad of 4 dense parameters -- a Philox block yields four words -- addressed into
// the image as fl_dp / fl_compress do; the 4 loads are issued before the peer loop, which walks
// the set bits of the round's mask (a wave-uniform trip count, K_r - 1 Philox blocks per quad).  An
// unsampled client and a round that is not live are left untouched; image padding is never
// written (it keeps the +0 the Adam kernel stored).  With K_r = 1 there is no pair and the
// quantised value is stored unmasked.  The clamp count of (client, round) is one integer atomicAdd
// per wave that counted any (integer addition does not depend on order).
//
// Open: one thread per float4 of the image for every K: only the running uint32 sum is live, the
// sources' loads are issued in batches of 8 before use.  A thread reads its coordinate from all K
// sources before it writes any of the n_dst destinations, which may be sources (in place: nobody
// else reads or writes that coordinate).  Image padding is written as exact 0 whatever the sources
// hold.  The metric tails behind the image, and the whole buffer of a round that is not live, are
// the fp32 left fold in source order (fl_robust.hip), so rounds past a stop stay exact no-ops.
//
// Launch- and latency-bound like fl_server and fl_robust: 64-thread workgroups; the tails run in
// workgroups of their own.  No float atomics, no LDS, no grid barrier, plain vector stores; no
// per-round host argument, so both launches are replayable.
#include "fl_common.h"
#include "fl_image.h"
#include "fl_philox.h"
#include "fl_secagg_open.h"

#define FL_SECAGG_THREADS 64
#define FL_SECAGG_BATCH 8

// Fixed-point image of a contribution: clamp(rint(c * 2^F), -L, L), +-inf -> +-L, NaN -> 0; `bad`: the
// coordinate was clamped or NaN.  The product is exact (a power of two) or inf; the compare is an integer one.
__device__ __forceinline__ int sa_quantize(float c, float scale, int L, bool& bad) {
    const float t = rintf(__fmul_rn(c, scale));
    if (t != t) { bad = true; return 0; }
    if (fabsf(t) >= 2147483648.f) { bad = true; return t < 0.f ? -L : L; }
    const int v = (int)t;  // exact: t is an integer below 2^31 in magnitude
    bad = v > L || v < -L;
    return v > L ? L : (v < -L ? -L : v);
}

__global__ void __launch_bounds__(FL_SECAGG_THREADS)
fl_secagg_mask_kernel(MLPDesc d, FLSecAgg p, float* const* __restrict__ bufs, uint32_t* const* __restrict__ clamp,
                      const FLState* __restrict__ st) {
    int r;
    const uint64_t mask = fl_round_gate(st, p.max_rounds, r) ? fl_round_mask(p.rtab, r) : 0;
    const int me = p.first_client + (int)blockIdx.y;
    if (!((mask >> me) & 1)) return;  // not live, or not sampled: the buffer stands (block-uniform)
    const int L = 0x7fffffff / __popcll(mask);
    float* __restrict__ comm = bufs[blockIdx.y];
    const int q = blockIdx.x * FL_SECAGG_THREADS + threadIdx.x;  // block of 4 dense parameters
    int cnt = 0;
    if (4 * q < d.P) {
        int j[4];
        float c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int di = 4 * q + k;
            j[k] = fl_image_index(d, di < d.P ? di : d.P - 1);
            c[k] = comm[j[k]];
        }
        // (a partial last quad re-read parameter P - 1 in its spare slots: neither counted nor stored)
        uint32_t y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bool bad;
            y[k] = (uint32_t)sa_quantize(c[k], p.scale, L, bad);
            cnt += (bad && 4 * q + k < d.P) ? 1 : 0;
        }
        for (uint64_t m = mask & ~(1ull << me); m; m &= m - 1) {
            const int o = __ffsll((unsigned long long)m) - 1;
            const int a = o > me ? me : o, b = o > me ? o : me;
            const uint4 w = philox4x32_10((uint32_t)q, (uint32_t)r, (uint32_t)(64 * a + b), FL_SECAGG_STREAM, p.key0,
                                          p.key1);
            if (o > me) { y[0] += w.x; y[1] += w.y; y[2] += w.z; y[3] += w.w; }
            else { y[0] -= w.x; y[1] -= w.y; y[2] -= w.z; y[3] -= w.w; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * q + k < d.P) comm[j[k]] = __uint_as_float(y[k]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (threadIdx.x == 0 && cnt) atomicAdd(&clamp[blockIdx.y][r], (uint32_t)cnt);
}

__global__ void __launch_bounds__(FL_SECAGG_THREADS)
fl_secagg_open_kernel(MLPDesc d, FLSecAgg p, const float* const* __restrict__ src, float* const* __restrict__ dst,
                      int n_dst, const FLState* __restrict__ st, int tails_len, int img_blocks) {
    if ((int)blockIdx.x >= img_blocks) {
        // metric tails: one float per thread, the left fold in source order
        const int j = ((int)blockIdx.x - img_blocks) * FL_SECAGG_THREADS + threadIdx.x;
        if (j >= tails_len) return;
        const float acc = fl_src_fold<FL_SECAGG_BATCH, FL_SECAGG_MAX_K>(src, p.K, d.Pimg + j);
        for (int q = 0; q < n_dst; ++q) dst[q][d.Pimg + j] = acc;
        return;
    }
    const int idx = 4 * (blockIdx.x * FL_SECAGG_THREADS + threadIdx.x);
    if (idx >= d.Pimg) return;
    int r;
    const uint64_t mask = fl_round_gate(st, p.max_rounds, r) ? fl_round_mask(p.rtab, r, p.K) : 0;
    uint32_t S[4] = {0u, 0u, 0u, 0u};
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < p.K; i0 += FL_SECAGG_BATCH) {
        float v[FL_SECAGG_BATCH][4];
        fl_src_load<FL_SECAGG_BATCH, 4>(src, p.K, i0, idx, v);
#pragma unroll
        for (int i = 0; i < FL_SECAGG_BATCH; ++i) {
            const bool in = i0 + i < p.K;
            const bool on = in && ((mask >> ((i0 + i) & 63)) & 1);
            sa_open_add(S, acc, v[i], i0 + i, in, on);  // (fl_secagg_open.h, shared with peer_allreduce.hip)
        }
    }
    float out[4];
    sa_open_finish(d, idx, mask, S, acc, p.inv_scale, out);
    for (int q = 0; q < n_dst; ++q) *reinterpret_cast<float4*>(dst[q] + idx) = make_float4(out[0], out[1], out[2], out[3]);
}

hipError_t fl_launch_secagg_mask(const MLPDesc& d, const FLSecAgg& p_in, float* const* bufs, int n,
                                 uint32_t* const* clamp, const FLState* st, hipStream_t s) {
    FLSecAgg p = p_in;
    if ((d.Pimg & 3) != 0 || d.P < 1 || !fl_secagg_scales(p) || bufs == nullptr || clamp == nullptr || st == nullptr ||
        p.rtab == nullptr || n < 1 || p.first_client < 0 || p.first_client + n > FL_SECAGG_MAX_K || p.max_rounds < 1)
        return hipErrorInvalidValue;
    const int quads = (d.P + 3) / 4;
    hipLaunchKernelGGL(fl_secagg_mask_kernel, dim3((quads + FL_SECAGG_THREADS - 1) / FL_SECAGG_THREADS, n),
                       dim3(FL_SECAGG_THREADS), 0, s, d, p, bufs, clamp, st);
    return hipGetLastError();
}

hipError_t fl_launch_secagg_open(const MLPDesc& d, const FLSecAgg& p_in, const float* const* src, float* const* dst,
                                 int n_dst, const FLState* st, int tails_len, hipStream_t s) {
    FLSecAgg p = p_in;
    if ((d.Pimg & 3) != 0 || d.Pimg < 4 || !fl_secagg_scales(p) || src == nullptr || dst == nullptr || st == nullptr ||
        p.rtab == nullptr || p.K < 1 || p.K > FL_SECAGG_MAX_K || n_dst < 1 || tails_len < 0 || p.max_rounds < 1)
        return hipErrorInvalidValue;
    const int img_blocks = (d.Pimg / 4 + FL_SECAGG_THREADS - 1) / FL_SECAGG_THREADS;
    const int tail_blocks = (tails_len + FL_SECAGG_THREADS - 1) / FL_SECAGG_THREADS;
    hipLaunchKernelGGL(fl_secagg_open_kernel, dim3(img_blocks + tail_blocks), dim3(FL_SECAGG_THREADS), 0, s, d, p, src,
                       dst, n_dst, st, tails_len, img_blocks);
    return hipGetLastError();
}
