// Block-scaled FP8 / FP4 update compression (OCP Microscaling, "MX": 32 elements share one E8M0 scale) with
// error feedback, in the compression slot behind the round's last Adam kernel, with the gate and the
// parity-buffered residual of fl_compress.hip.  With x the image the round trained from, e the client's
// residual, w its FedAvg weight (rtab), on the P real parameters, every operation one fp32 rounding:
//
//   u  = (local - x) + e
//   c  = C(u)                                   e' = error_feedback ? u - c : 0
//   contribution = w * (x + c)                  image padding is never read or written
//
// C works on blocks of 32 consecutive dense parameters (the last one partial).  A = the largest
// bits(u) & 0x7fffffff of the block, E = A >> 23:
//   E == 255 (an inf or NaN in the block): the block travels raw, c = u, e' = 0
//   E <  32  (block maximum below 2^-95) : c = copysign(0, u)
//   else e = E - 127 - emax (emax = 8 / 15 / 2 for e4m3 / e5m2 / e2m1), t = |u| 2^-e, q = t rounded into the
//        format's non-negative finite values (saturating at the maximum 448 / 57344 / 6), c = copysign(q 2^e, u).
// Rounding: nearest with ties to the even element code, or stochastic: with l <= t < h the neighbouring grid
// values, q = ((word >> 8) < (t - l) / (h - l) 2^24) ? h : l, word = word p % 4 of Philox4x32-10 at counter
// (p / 4, round, client, FL_MX_STREAM).  The cut-off at E = 32 keeps every scale and every dequantised value a
// normal fp32.  The statistic is the largest 2^e of the round's quantised blocks (0: none).
// fedmi/fl/compress.py mx_quantize is the host model, written from the formats' value tables.
//
// Geometry.  The rule is local to a block, so nothing is recomputed per workgroup and nothing goes through
// LDS: one thread owns one quad of dense parameters -- one Philox block -- and issues its 12 loads (local, x,
// residual, clamped into the model) before the first use; 8 consecutive lanes hold one MX block and find its
// maximum with three xor shuffles (4, 2, 1) over the integer keys, so a wave covers 8 blocks and a workgroup of
// 256 threads 32.  No barrier, no atomics, no LDS in these workgroups.  Contribution and residual leave as one
// 16-byte store each where the quad is one aligned float4 of the image, float by float where it straddles a
// row, a layer or the model's end.  One more workgroup, the grid's last, walks all quads again for the
// statistic: an integer max of the finite blocks' E over its lanes, waves (4 LDS words) -- no float sum.
//
// Conversion.  The integer path takes the quotient and remainder of the 24-bit significand by the grid step
// at |u|'s binade (the subnormal range widens the shift) and rounds on the remainder.  The hardware path
// (nearest only) clamps |u| to max 2^e in integers, converts a pair with v_cvt_scalef32_pk_{fp8,bf8,fp4}_f32
// and back with v_cvt_scalef32_pk_f32_{fp8,bf8,fp4}, the scale operand 2^e as a float.  mx_conv_default says
// which (format, rounding) runs on which; docs/ARCHITECTURE.md has the evidence.
#include "fl_common.h"
#include "fl_device.h"
#include "fl_image.h"
#include "fl_philox.h"

#define FL_MX_THREADS 256
#define FL_MX_LANES (FL_MX_BLOCK / 4)  // lanes (quads) of one MX block

// One rounding per operation whatever the flags (as fl_lowrank.hip's helpers).
#pragma clang fp contract(off)
__device__ __forceinline__ float mx_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float mx_add(float a, float b) { return a + b; }
__device__ __forceinline__ float mx_sub(float a, float b) { return a - b; }

// An element format: mantissa bits, exponent of the largest binade, exponent of the smallest normal binade,
// and the fp32 mantissa field of the largest value (1.75 2^emax for the FP8 formats, whose top code is not a
// number or infinite; 1.5 2^emax for FP4).
template <int FMT> struct MxFmt;
template <> struct MxFmt<FL_MX_E4M3> { static constexpr int M = 3, EMAX = 8, EMIN = -6; static constexpr uint32_t TOP = 0x600000u; };
template <> struct MxFmt<FL_MX_E5M2> { static constexpr int M = 2, EMAX = 15, EMIN = -14; static constexpr uint32_t TOP = 0x600000u; };
template <> struct MxFmt<FL_MX_E2M1> { static constexpr int M = 1, EMAX = 2, EMIN = 0; static constexpr uint32_t TOP = 0x400000u; };

__host__ __device__ constexpr int mx_emax(int fmt) { return fmt == FL_MX_E4M3 ? 8 : fmt == FL_MX_E5M2 ? 15 : 2; }
__host__ __device__ constexpr int mx_bits(int fmt) { return fmt == FL_MX_E2M1 ? 4 : 8; }

// Which conversion a (format, rounding) pair runs on when FLMx::conv leaves the choice here: the hardware
// conversion only where it reproduced the rule bit for bit on the grid inputs of tests/test_compress_mx.py.
__host__ __device__ constexpr bool mx_conv_default(int fmt, bool stochastic) {
    return !stochastic && (fmt == FL_MX_E4M3 || fmt == FL_MX_E5M2 || fmt == FL_MX_E2M1);
}

// |c| of one element by integer arithmetic: `ub` = bits of |u| (finite, block exponent E in 32 .. 254).
template <int FMT, bool SR>
__device__ __forceinline__ float mx_quant_int(uint32_t ub, int E, uint32_t word) {
    using F = MxFmt<FMT>;
    const uint32_t top = ((uint32_t)E << 23) | F::TOP;  // max 2^e
    if (ub >= top) return __uint_as_float(top);         // the band [max, 2^(emax + 1)) saturates
    const int Eu = (int)(ub >> 23), Ee = Eu ? Eu : 1;
    const uint64_t sig = (ub & 0x7fffffu) | (Eu ? 0x800000u : 0u);  // |u| = sig 2^(Ee - 150)
    const int k = Ee - E + F::EMAX;            // t's binade (a denormal u: an upper bound, far below EMIN)
    const int kk = k > F::EMIN ? k : F::EMIN;  // the grid step at t is 2^(kk - M)
    int sh = 23 - F::M + (kk - k);             // t = sig 2^-sh steps
    sh = sh < 63 ? sh : 63;                    // (sig < 2^24: from 2^-39 of a step down nothing changes)
    uint32_t q = (uint32_t)(sig >> sh);
    const uint64_t rem = sig & ((1ull << sh) - 1ull);
    bool up;
    if constexpr (SR) {  // (word >> 8) < rem 2^-sh 2^24, both sides exact
        const uint64_t w24 = word >> 8;
        up = sh <= 24 ? w24 < (rem << (24 - sh)) : (w24 << (sh - 24)) < rem;
    } else {             // q's low bit is the low bit of the element code
        const uint64_t half = 1ull << (sh - 1);
        up = rem > half || (rem == half && (q & 1u));
    }
    q += up ? 1u : 0u;
    // q steps of 2^(kk - M) 2^e: exact, zero or a normal fp32 (the step's exponent field is 1 .. 254)
    return mx_mul((float)q, __uint_as_float((uint32_t)(kk - F::M + E - F::EMAX) << 23));
}

typedef short mx_v2s __attribute__((ext_vector_type(2)));
typedef float mx_v2f __attribute__((ext_vector_type(2)));

// |c| of a pair by the scaled conversion instructions, nearest: `a0`, `a1` = |u| clamped to max 2^e, `scale`
// = 2^e as a float.
template <int FMT>
__device__ __forceinline__ void mx_quant_hw(float a0, float a1, float scale, float& c0, float& c1) {
    mx_v2f o;
    if constexpr (FMT == FL_MX_E4M3) {
        const mx_v2s z = {0, 0};
        const mx_v2s code = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(z, a0, a1, scale, false);
        o = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((uint32_t)(uint16_t)code.x, scale, false);
    } else if constexpr (FMT == FL_MX_E5M2) {
        const mx_v2s z = {0, 0};
        const mx_v2s code = __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(z, a0, a1, scale, false);
        o = __builtin_amdgcn_cvt_scalef32_pk_f32_bf8((uint32_t)(uint16_t)code.x, scale, false);
    } else {
        const uint32_t code = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0u, a0, a1, scale, 0);
        o = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(code & 0xffu, scale, 0);
    }
    c0 = o.x;
    c1 = o.y;
}

// A thread's quad: image positions (clamped into the model), the three inputs, u and the integer maximum of
// its real entries' magnitudes.
struct MxQuad {
    int j[4];
    float x[4], u[4];
    uint32_t amax;
};
__device__ __forceinline__ void mx_load(const MLPDesc& d, int qd, const float* __restrict__ local,
                                        const float* __restrict__ pg, const float* __restrict__ ein, MxQuad& v) {
    const int P = d.P;
    float a[4], e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int di = 4 * qd + i;
        v.j[i] = fl_image_index(d, di < P ? di : P - 1);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { a[i] = local[v.j[i]]; v.x[i] = pg[v.j[i]]; e[i] = ein[v.j[i]]; }
    v.amax = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v.u[i] = mx_add(mx_sub(a[i], v.x[i]), e[i]);
        const uint32_t ub = __float_as_uint(v.u[i]) & 0x7fffffffu;
        if (4 * qd + i < P && ub > v.amax) v.amax = ub;
    }
}
// The block's maximum: the 8 lanes of a block are consecutive and 8-aligned in the wave.
__device__ __forceinline__ uint32_t mx_block_max(uint32_t a) {
#pragma unroll
    for (int off = FL_MX_LANES / 2; off; off >>= 1) {
        const uint32_t t = (uint32_t)__shfl_xor((int)a, off, 64);
        a = t > a ? t : a;
    }
    return a;
}

template <int FMT, bool SR, bool HW>
__global__ void __launch_bounds__(FL_MX_THREADS)
fl_mx_kernel(MLPDesc d, FLMx p, const float* __restrict__ local, const float* __restrict__ pg,
             float* __restrict__ comm, const FLState* __restrict__ st, const float* __restrict__ rtab) {
    static_assert(!(SR && HW), "the stochastic rule runs on integer code");
    __shared__ int wmax[FL_MX_THREADS / 64];  // (the statistic's workgroup alone)
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;
    const float w = fl_round_weight(rtab, r);
    const int P = d.P, tid = threadIdx.x;
    const int nq = (P + 3) >> 2;
    const float* __restrict__ ein = p.residual + (size_t)(r & 1) * d.Pimg;
    float* __restrict__ eout = p.residual + (size_t)((r + 1) & 1) * d.Pimg;

    if (blockIdx.x == gridDim.x - 1) {  // the statistic: the largest E of the finite blocks with E >= 32
        if (w == 0.f) {
            if (tid == 0) p.stat_hist[r] = 0.f;
            return;
        }
        int best = 0;
        const int per = (nq + FL_MX_THREADS - 1) / FL_MX_THREADS;
        for (int it = 0; it < per; ++it) {  // (a trip's quads start at a multiple of 256: blocks stay lane-aligned)
            MxQuad v;
            mx_load(d, it * FL_MX_THREADS + tid, local, pg, ein, v);
            const int E = (int)(mx_block_max(v.amax) >> 23);
            best = E != 255 && E > best ? E : best;
        }
#pragma unroll
        for (int off = 32; off >= FL_MX_LANES; off >>= 1) {
            const int t = __shfl_xor(best, off, 64);
            best = t > best ? t : best;
        }
        if ((tid & 63) == 0) wmax[tid >> 6] = best;
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int i = 1; i < FL_MX_THREADS / 64; ++i) best = wmax[i] > best ? wmax[i] : best;
            p.stat_hist[r] = best >= 32 ? __uint_as_float((uint32_t)(best - mx_emax(FMT)) << 23) : 0.f;
        }
        return;
    }

    const int qd = blockIdx.x * FL_MX_THREADS + tid;
    if (w == 0.f) {  // not sampled: the Adam kernel's zeros stay; the residual carries over to the next half
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int di = 4 * qd + i;
            if (di < P) {
                const int j = fl_image_index(d, di);
                eout[j] = ein[j];
            }
        }
        return;
    }
    MxQuad v;
    mx_load(d, qd, local, pg, ein, v);
    const int E = (int)(mx_block_max(v.amax) >> 23);
    if (qd >= nq) return;  // (behind the shuffles: a block's lanes past P took part with 0)

    float c[4], en[4];
    if (E == 255) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { c[i] = v.u[i]; en[i] = 0.f; }
    } else {
        if (E < 32) {
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = 0.f;
        } else if constexpr (HW) {
            const uint32_t top = ((uint32_t)E << 23) | MxFmt<FMT>::TOP;
            const float scale = __uint_as_float((uint32_t)(E - MxFmt<FMT>::EMAX) << 23);
            float a[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t ub = __float_as_uint(v.u[i]) & 0x7fffffffu;
                a[i] = __uint_as_float(ub < top ? ub : top);
            }
            mx_quant_hw<FMT>(a[0], a[1], scale, c[0], c[1]);
            mx_quant_hw<FMT>(a[2], a[3], scale, c[2], c[3]);
        } else {
            uint32_t wd[4] = {0u, 0u, 0u, 0u};
            if constexpr (SR) {
                const uint4 o = philox4x32_10((uint32_t)qd, (uint32_t)r, (uint32_t)p.client, FL_MX_STREAM, p.key0, p.key1);
                wd[0] = o.x; wd[1] = o.y; wd[2] = o.z; wd[3] = o.w;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                c[i] = mx_quant_int<FMT, SR>(__float_as_uint(v.u[i]) & 0x7fffffffu, E, wd[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            c[i] = copysignf(c[i], v.u[i]);
            en[i] = p.error_feedback ? mx_sub(v.u[i], c[i]) : 0.f;
        }
    }
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = mx_mul(w, mx_add(v.x[i], c[i]));
    const int j0 = v.j[0];
    if (4 * qd + 3 < P && (j0 & 3) == 0 && v.j[1] == j0 + 1 && v.j[2] == j0 + 2 && v.j[3] == j0 + 3) {
        *reinterpret_cast<float4*>(comm + j0) = make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<float4*>(eout + j0) = make_float4(en[0], en[1], en[2], en[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * qd + i < P) {
                comm[v.j[i]] = o[i];
                eout[v.j[i]] = en[i];
            }
    }
}

long long fl_mx_uplink_bytes(int P, int fmt) {
    return ((long long)P + FL_MX_BLOCK - 1) / FL_MX_BLOCK + ((long long)P * mx_bits(fmt) + 7) / 8;
}

template <int FMT>
static void mx_launch_fmt(bool sr, bool hw, dim3 grid, const MLPDesc& d, const FLMx& p, const float* local,
                          const float* pg, float* comm, const FLState* st, const float* rtab, hipStream_t s) {
    const dim3 block(FL_MX_THREADS);
    if (sr)
        hipLaunchKernelGGL((fl_mx_kernel<FMT, true, false>), grid, block, 0, s, d, p, local, pg, comm, st, rtab);
    else if (hw)
        hipLaunchKernelGGL((fl_mx_kernel<FMT, false, true>), grid, block, 0, s, d, p, local, pg, comm, st, rtab);
    else
        hipLaunchKernelGGL((fl_mx_kernel<FMT, false, false>), grid, block, 0, s, d, p, local, pg, comm, st, rtab);
}

hipError_t fl_launch_mx(const MLPDesc& d, const FLMx& p, const float* local, const float* pg, float* comm,
                        const FLState* st, const float* rtab, hipStream_t s) {
    if ((d.Pimg & 3) != 0 || d.P < 1 || p.fmt < FL_MX_E4M3 || p.fmt > FL_MX_E2M1 || p.conv < -1 || p.conv > 1 ||
        (p.conv == 1 && p.stochastic) || p.residual == nullptr || p.stat_hist == nullptr || p.max_rounds < 1 ||
        local == nullptr || pg == nullptr || comm == nullptr || st == nullptr || rtab == nullptr)
        return hipErrorInvalidValue;
    const bool sr = p.stochastic != 0;
    const bool hw = p.conv < 0 ? mx_conv_default(p.fmt, sr) : p.conv == 1;
    const int quads = (d.P + 3) / 4;
    const dim3 grid((quads + FL_MX_THREADS - 1) / FL_MX_THREADS + 1);  // + the statistic's workgroup
    if (p.fmt == FL_MX_E4M3) mx_launch_fmt<FL_MX_E4M3>(sr, hw, grid, d, p, local, pg, comm, st, rtab, s);
    else if (p.fmt == FL_MX_E5M2) mx_launch_fmt<FL_MX_E5M2>(sr, hw, grid, d, p, local, pg, comm, st, rtab, s);
    else mx_launch_fmt<FL_MX_E2M1>(sr, hw, grid, d, p, local, pg, comm, st, rtab, s);
    return hipGetLastError();
}
