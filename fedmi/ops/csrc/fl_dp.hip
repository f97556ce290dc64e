// Client-level differential privacy of a FedAvg round (DP-FedAvg with distributed noise): one
// launch per round, after the last local step's Adam kernel, rewrites the parameter image of the
// round's FedAvg contribution in the comm buffer.  With x the image the round trained from, the
// update D = local - x, the FedAvg weight w (rtab) and the round's noise scale sigma (host table):
//
//   c            = min(1, S / ||D||_2)               (||D|| = 0 -> c = 1)
//   contribution = w * (x + c D) + sigma * N(0, I)   on real parameters; image padding stays 0
//
// An unclipped round (c = 1) contributes w * local exactly as the Adam kernel stored it.  A round
// that is not live, and a client that is not sampled (w = 0), are left untouched (no noise).
//
// Every workgroup recomputes the whole ||D||^2 (both images come from L2; no grid barrier) in ONE
// fixed order -- per thread the float4s t, t + 1024, ... of the image, an xor tree over the wave,
// the 16 waves' sums in wave order -- so all workgroups hold a bit-identical c and a run is
// bitwise repeatable.  Image padding is zero in both images and adds exact zeros.
//
// Noise: dense parameter p draws lane p % 4 of Philox4x32-10 at counter (p / 4, round, rank,
// 0x46454450) under the engine's 64-bit key; u = u01(output); Box-Muller on (u0, u1) gives lanes
// 0 (cos) and 1 (sin), on (u2, u3) lanes 2 and 3, with the full-precision logf / sincosf.  The
// round index is the device state's cur_round: a replayed graph draws fresh noise every round.
// fedmi/privacy/philox.py is the host model of the stream.
#include "fl_common.h"
#include "fl_device.h"
#include "fl_image.h"
#include "fl_philox.h"
#include <math.h>

#define FL_DP_THREADS 1024

__global__ void __launch_bounds__(FL_DP_THREADS)
fl_dp_kernel(MLPDesc d, FLDp p, const float* __restrict__ local, const float* __restrict__ pg,
             float* __restrict__ comm, const FLState* __restrict__ st, const float* __restrict__ rtab) {
    __shared__ float wsum[FL_DP_THREADS / 64];
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;  // past a stop / max_rounds: the Adam kernel republished the global image
    const float w = fl_round_weight(rtab, r);
    if (w == 0.f) {  // not sampled this round: zeros from the Adam kernel, no noise
        if (blockIdx.x == 0 && threadIdx.x == 0) p.norm_hist[r] = 0.f;
        return;
    }
    float acc = 0.f;
    const float4* l4 = reinterpret_cast<const float4*>(local);
    const float4* g4 = reinterpret_cast<const float4*>(pg);
    for (int i = threadIdx.x; i < (d.Pimg >> 2); i += FL_DP_THREADS) {
        const float4 a = l4[i], x = g4[i];
        const float d0 = a.x - x.x, d1 = a.y - x.y, d2 = a.z - x.z, d3 = a.w - x.w;
        acc = __fmaf_rn(d0, d0, acc);
        acc = __fmaf_rn(d1, d1, acc);
        acc = __fmaf_rn(d2, d2, acc);
        acc = __fmaf_rn(d3, d3, acc);
    }
    const float nrm = sqrtf(block_sum_ordered<FL_DP_THREADS>(acc, wsum));
    if (blockIdx.x == 0 && threadIdx.x == 0) p.norm_hist[r] = nrm;
    const bool clipped = nrm > p.clip;
    if (!clipped && !p.noise) return;  // the Adam kernel's w * local stands
    const float cc = clipped ? p.clip / nrm : 1.f;

    const int q = blockIdx.x * FL_DP_THREADS + threadIdx.x;  // block of 4 dense parameters
    if (4 * q >= d.P) return;
    float nz[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.noise) {
        const uint4 o = philox4x32_10((uint32_t)q, (uint32_t)r, (uint32_t)p.rank, 0x46454450u, p.key0, p.key1);
        const float sigma = p.sigma[r];
        const float r0 = sqrtf(-2.f * logf(u01(o.x))), r1 = sqrtf(-2.f * logf(u01(o.z)));
        float s0, c0, s1, c1;
        sincosf(6.2831853071795864769f * u01(o.y), &s0, &c0);
        sincosf(6.2831853071795864769f * u01(o.w), &s1, &c1);
        nz[0] = __fmul_rn(sigma, __fmul_rn(r0, c0));
        nz[1] = __fmul_rn(sigma, __fmul_rn(r0, s0));
        nz[2] = __fmul_rn(sigma, __fmul_rn(r1, c1));
        nz[3] = __fmul_rn(sigma, __fmul_rn(r1, s1));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int di = 4 * q + k;
        if (di >= d.P) break;
        const int j = fl_image_index(d, di);
        float t = local[j];
        if (clipped) {
            const float x = pg[j];
            t = __fmaf_rn(cc, __fsub_rn(t, x), x);
        }
        comm[j] = p.noise ? __fmaf_rn(w, t, nz[k]) : __fmul_rn(w, t);
    }
}

hipError_t fl_launch_dp(const MLPDesc& d, const FLDp& p, const float* local, const float* pg, float* comm,
                        const FLState* st, const float* rtab, hipStream_t s) {
    if ((d.Pimg & 3) != 0 || !(p.clip > 0.f) || p.sigma == nullptr || p.norm_hist == nullptr || p.max_rounds < 1)
        return hipErrorInvalidValue;
    const int quads = (d.P + 3) / 4;
    hipLaunchKernelGGL(fl_dp_kernel, dim3((quads + FL_DP_THREADS - 1) / FL_DP_THREADS), dim3(FL_DP_THREADS), 0, s,
                       d, p, local, pg, comm, st, rtab);
    return hipGetLastError();
}
