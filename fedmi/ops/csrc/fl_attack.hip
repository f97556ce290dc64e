// Byzantine attack models of a FedAvg round: one launch per round, after the K clients published their
// contributions (local steps, then any DP or compression kernel: a Byzantine client obeys neither) and
// before the screen, the robust rule, the secure-aggregation mask and the sum, rewrites the contributions
// of the round's bad sampled clients in place.  fedmi/fl/attack.py is the specification and attack_model
// the host model, bit for bit except the normal of FL_ATTACK_GAUSS.  With S_r the round's sampled clients
// (rtab mask of the round in `st`), B_r = S_r & bad, H_r = S_r & ~bad, w_j client j's FedAvg weight in its
// buffer (row r of wtab; null: 1), x the image the round trained from and m_j[p] = div(c_j[p], w_j) the
// model behind contribution c_j, every k in B_r gets c_k[p] = mul(w_k, a_k[p]) on the real parameters p:
//
//   sign-flip   a_k = sub(x, mul(s, sub(m_k, x)))                        its own update reversed and scaled
//   gauss       a_k = add(m_k, mul(sigma, n_k[p]))
//   alie        mu  = div(sum_{j in H_r} m_j, float(|H_r|))              sums from +0 in client order
//               var = |H_r| >= 2 ? div(sum_{j in H_r} mul(d_j, d_j), float(|H_r| - 1)) : 0,  d_j = sub(m_j, mu)
//               a_k = sub(mu, mul(z, sqrt(var)))                         (Baruch et al. 2019, "A Little Is Enough")
//   ipm         a_k = sub(x, mul(eps, sub(mu, x)))                       (Xie et al. 2020, inner-product manipulation)
//
// Every operation is one round-to-nearest fp32 operation (sqrtf: correctly rounded).  The sums, differences
// and products go through attack_add / attack_sub / attack_mul below, defined with contraction off: the
// header's __fadd_rn / __fsub_rn / __fmul_rn are plain operators compiled where contraction is allowed, and a
// product feeding a difference (x - s t) was fused into one fma, one rounding where the rule has two (as in
// fl_geomed.hip).  Without a weight table the divisions and the final product are not issued:
// by 1.0 they are exact.
//
// Never written: image padding (it stays what it is, exact 0), the metric tails behind the image, honest
// and unsampled clients' buffers; nothing at all in a round that is not live (past an early stop or past
// max_rounds: it stays the exact no-op it is), with B_r empty, and for alie / ipm with H_r empty.
//
// Two kernel shapes.  The colluding kinds (alie, ipm) need every honest client's value of a coordinate:
// one thread owns a coordinate of the image, laid out like fl_robust_kernel -- K buckets 4 / 8 / 16 / 32 /
// 64 with every loop unrolled, so the K values stay in registers; one float4 of the image per thread up to
// 8, one float above; every load issued before the first use (fl_src_load); slots past K re-read source
// K - 1 and carry no mask bit.  The real-parameter predicate is fl_image_lim's.  The own-buffer kinds
// (sign-flip, gauss) need only the client's own value: one thread owns a quad of DENSE parameters, mapped to
// the image through fl_image_index as fl_dp_kernel does -- the quad is the Philox block of gauss -- and
// loops over the bad sampled clients.
//
// gauss: dense parameter p draws lane p % 4 of Philox4x32-10 at counter (p / 4, round, k, FL_ATTACK_STREAM)
// under the 64-bit attack seed; u = u01(output); Box-Muller on (u0, u1) gives lanes 0 (cos) and 1 (sin), on
// (u2, u3) lanes 2 and 3, with the full-precision logf / sincosf, exactly as fl_dp.hip evaluates the DP
// noise.  The round index is the device state's cur_round: a replayed graph draws fresh noise every round.
//
// No LDS, no atomics, no grid barrier; plain vector stores only.  No per-round host argument: the launch
// is capturable like fl_robust's.
#include "fl_common.h"
#include "fl_image.h"
#include "fl_philox.h"
#include <cmath>

#pragma clang fp contract(off)
__device__ __forceinline__ float attack_add(float a, float b) { return a + b; }
__device__ __forceinline__ float attack_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float attack_mul(float a, float b) { return a * b; }

#define FL_ATTACK_THREADS 64        // colluding kinds: as fl_robust (launch- and latency-bound)
#define FL_ATTACK_OWN_THREADS 256   // own-buffer kinds: quads of dense parameters

template <int KB, int VEC, bool WEIGHTED>
__global__ void __launch_bounds__(FL_ATTACK_THREADS)
fl_attack_collude_kernel(MLPDesc d, FLAttack p, float* const* __restrict__ bufs, const float* __restrict__ x,
                         const FLState* __restrict__ st) {
    const int u = blockIdx.x * FL_ATTACK_THREADS + threadIdx.x;
    const int idx = VEC * u;
    if (idx >= d.Pimg) return;
    float v[KB][VEC];
    fl_src_load<KB, VEC>(bufs, p.K, 0, idx, v);
    float xv[VEC];
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(x + idx);
        xv[0] = t.x; xv[1] = t.y; xv[2] = t.z; xv[3] = t.w;
    } else {
        xv[0] = x[idx];
    }
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;
    const uint64_t mask = fl_round_mask(p.rtab, r, p.K);
    const uint64_t B = mask & p.bad, H = mask & ~p.bad;
    if (B == 0 || H == 0) return;
    // real parameters among this thread's floats: elements [0, lim) of its float4 / its one float
    const int lim4 = fl_image_lim(d, idx & ~3);
    const int lim = VEC == 4 ? lim4 : (lim4 > (idx & 3) ? 1 : 0);
    if (lim <= 0) return;
    const float* wr = WEIGHTED ? p.wtab + (size_t)r * p.K : nullptr;
    const int nH = __popcll(H);

    // the honest clients' models, in place of their contributions, and their sum in client order from +0
    float mu[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) mu[e] = 0.f;
#pragma unroll
    for (int i = 0; i < KB; ++i) {
        if (!((H >> i) & 1)) continue;   // (uniform)
        float w = 1.f;
        if constexpr (WEIGHTED) w = wr[i];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if constexpr (WEIGHTED) v[i][e] = __fdiv_rn(v[i][e], w);
            mu[e] = attack_add(mu[e], v[i][e]);
        }
    }
    float a[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) mu[e] = __fdiv_rn(mu[e], (float)nH);
    if (p.kind == FL_ATTACK_ALIE) {
        float var[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) var[e] = 0.f;
        if (nH >= 2) {
#pragma unroll
            for (int i = 0; i < KB; ++i) {
                if (!((H >> i) & 1)) continue;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float df = attack_sub(v[i][e], mu[e]);
                    var[e] = attack_add(var[e], attack_mul(df, df));
                }
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) var[e] = __fdiv_rn(var[e], (float)(nH - 1));
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] = attack_sub(mu[e], attack_mul(p.z, sqrtf(var[e])));
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] = attack_sub(xv[e], attack_mul(p.scale, attack_sub(mu[e], xv[e])));
    }

    // the same vector into every bad sampled client's buffer, scaled by that client's weight
#pragma unroll
    for (int i = 0; i < KB; ++i) {
        if (!((B >> i) & 1)) continue;   // (uniform; slots past K carry no bit)
        float* o = bufs[i] + idx;
        float c[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            c[e] = a[e];
            if constexpr (WEIGHTED) c[e] = attack_mul(wr[i], a[e]);
        }
        if constexpr (VEC == 4) {
            if (lim >= 4) {
                *reinterpret_cast<float4*>(o) = make_float4(c[0], c[1], c[2], c[3]);
            } else {   // a float4 that ends in image padding: the padding is not written
                o[0] = c[0];
                if (lim > 1) o[1] = c[1];
                if (lim > 2) o[2] = c[2];
            }
        } else {
            *o = c[0];
        }
    }
}

template <bool WEIGHTED>
__global__ void __launch_bounds__(FL_ATTACK_OWN_THREADS)
fl_attack_own_kernel(MLPDesc d, FLAttack p, float* const* __restrict__ bufs, const float* __restrict__ x,
                     const FLState* __restrict__ st) {
    const int q = blockIdx.x * FL_ATTACK_OWN_THREADS + threadIdx.x;   // block of 4 dense parameters
    if (4 * q >= d.P) return;
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;
    const uint64_t B = fl_round_mask(p.rtab, r, p.K) & p.bad;
    if (B == 0) return;
    int j[4];
    float xv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int di = 4 * q + e < d.P ? 4 * q + e : d.P - 1;   // (past the last parameter: read, never written)
        j[e] = fl_image_index(d, di);
        xv[e] = x[j[e]];
    }
    for (uint64_t rest = B; rest != 0; rest &= rest - 1) {
        const int k = __ffsll((unsigned long long)rest) - 1;
        float* c = bufs[k];
        float w = 1.f;
        if constexpr (WEIGHTED) w = p.wtab[(size_t)r * p.K + k];
        float nz[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.kind == FL_ATTACK_GAUSS) {
            const uint4 o = philox4x32_10((uint32_t)q, (uint32_t)r, (uint32_t)k, FL_ATTACK_STREAM, p.key0, p.key1);
            const float r0 = sqrtf(-2.f * logf(u01(o.x))), r1 = sqrtf(-2.f * logf(u01(o.z)));
            float s0, c0, s1, c1;
            sincosf(6.2831853071795864769f * u01(o.y), &s0, &c0);
            sincosf(6.2831853071795864769f * u01(o.w), &s1, &c1);
            nz[0] = attack_mul(p.scale, attack_mul(r0, c0));
            nz[1] = attack_mul(p.scale, attack_mul(r0, s0));
            nz[2] = attack_mul(p.scale, attack_mul(r1, c1));
            nz[3] = attack_mul(p.scale, attack_mul(r1, s1));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (4 * q + e >= d.P) break;
            float m = c[j[e]];
            if constexpr (WEIGHTED) m = __fdiv_rn(m, w);
            float a;
            if (p.kind == FL_ATTACK_GAUSS) a = attack_add(m, nz[e]);
            else a = attack_sub(xv[e], attack_mul(p.scale, attack_sub(m, xv[e])));
            if constexpr (WEIGHTED) a = attack_mul(w, a);
            c[j[e]] = a;
        }
    }
}

template <int KB, int VEC>
static void collude_launch(const MLPDesc& d, const FLAttack& p, float* const* bufs, const float* x, const FLState* st,
                           hipStream_t s) {
    const int units = d.Pimg / VEC;
    const int blocks = (units + FL_ATTACK_THREADS - 1) / FL_ATTACK_THREADS;
    if (p.wtab != nullptr)
        hipLaunchKernelGGL((fl_attack_collude_kernel<KB, VEC, true>), dim3(blocks), dim3(FL_ATTACK_THREADS), 0, s, d, p,
                           bufs, x, st);
    else
        hipLaunchKernelGGL((fl_attack_collude_kernel<KB, VEC, false>), dim3(blocks), dim3(FL_ATTACK_THREADS), 0, s, d, p,
                           bufs, x, st);
}

hipError_t fl_launch_attack(const MLPDesc& d, const FLAttack& p, float* const* bufs, const float* x, const FLState* st,
                            hipStream_t s) {
    if ((d.Pimg & 3) != 0 || d.Pimg < 4 || d.P < 1 || bufs == nullptr || x == nullptr || st == nullptr ||
        p.rtab == nullptr || p.K < 1 || p.K > FL_ATTACK_MAX_K || p.max_rounds < 1 || p.kind < FL_ATTACK_SIGN_FLIP ||
        p.kind > FL_ATTACK_IPM || !(p.scale > 0.f) || !std::isfinite(p.scale) || !std::isfinite(p.z))
        return hipErrorInvalidValue;
    if (p.kind == FL_ATTACK_SIGN_FLIP || p.kind == FL_ATTACK_GAUSS) {
        const int quads = (d.P + 3) / 4;
        const int blocks = (quads + FL_ATTACK_OWN_THREADS - 1) / FL_ATTACK_OWN_THREADS;
        if (p.wtab != nullptr)
            hipLaunchKernelGGL(fl_attack_own_kernel<true>, dim3(blocks), dim3(FL_ATTACK_OWN_THREADS), 0, s, d, p, bufs, x, st);
        else
            hipLaunchKernelGGL(fl_attack_own_kernel<false>, dim3(blocks), dim3(FL_ATTACK_OWN_THREADS), 0, s, d, p, bufs, x, st);
        return hipGetLastError();
    }
    if (p.K <= 4) collude_launch<4, 4>(d, p, bufs, x, st, s);
    else if (p.K <= 8) collude_launch<8, 4>(d, p, bufs, x, st, s);
    else if (p.K <= 16) collude_launch<16, 1>(d, p, bufs, x, st, s);
    else if (p.K <= 32) collude_launch<32, 1>(d, p, bufs, x, st, s);
    else collude_launch<64, 1>(d, p, bufs, x, st, s);
    return hipGetLastError();
}
