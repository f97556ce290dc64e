// Server optimizer of a FedAvg round (FedAvgM: Hsu et al. 2019; FedAdagrad / FedAdam / FedYogi:
// Reddi et al. 2021, Algorithm 2): one launch per round, after the round's aggregated image `a`
// is complete (all-reduced, so after any DP clip + noise), replaces it in place by the new global
// image.  With x the image the round trained from and d = a - x the pseudo-gradient:
//
//   sgd     : m = b1 m + d                                     new = x + lr m
//   adagrad : m = b1 m + (1 - b1) d   v = v + d^2              new = x + lr m / (sqrt(v) + tau)
//   adam    : same m                  v = b2 v + (1 - b2) d^2  same step
//   yogi    : same m                  v = v - (1 - b2) d^2 sign(v - d^2)   same step
//
// m starts at 0 and v at tau^2 (caller-owned fp32 images); no bias correction.  The step is the same
// replicated computation on every rank: every operation is an explicit round-to-nearest fp32
// intrinsic (no contraction, no fast division), so the result is bit-identical on all ranks and
// across graph replays whatever the compile flags.  Exactly, per element:
//
//   d  = sub(a, x)
//   m' = fma(b1, m, d)                      (sgd)      fma(b1, m, mul(1 - b1, d))   (adaptive)
//   v' = fma(d, d, v)                       (adagrad)
//        fma(b2, v, mul(1 - b2, mul(d, d))) (adam)
//        v -/+ mul(1 - b2, mul(d, d)) by the sign of sub(v, mul(d, d)), v when that is 0   (yogi)
//   new = fma(lr, m', x)                    (sgd)      fma(lr, div(m', add(sqrt(v'), tau)), x)
//
// Image padding (rows >= N, columns >= K, the 4 pad floats of a row, bias slots >= N) keeps its
// values: 0 in the image and in m, tau^2 in v (Adam's v would decay there otherwise).  The metric
// tails behind the image are never touched.  A round that is not live (past an early stop or past
// max_rounds) changes neither the image nor m / v.
//
// The kernel is launch- and latency-bound (a few thousand float4s over four arrays, all from L2):
// one 64-thread workgroup per 64 work items, so the ~50-75 waves land on CUs of their own instead of
// queueing on one, and every thread issues all of its loads before the first use (one L2 latency
// per thread, no loop).  No grid barrier, no atomics, plain vector stores.
//
//   fp32 mode: one thread per float4 of the image.
//   bf16 mode: one thread per 8-element item / bias slot of the packed split-bf16 parameter region
//     (the index math of fl_pack_bf16_body, fl_kernels_bf16.hip): the same launch writes the hi and
//     lo images of the new global model into pk_global, which the next train kernel stages, so no
//     stand-alone pack runs.  Items outside the fp32 image write zeros, as the pack kernel does.
//     A round that is not live packs `a` as it stands (the republished global image), so the packed
//     image always matches the fp32 image the next round reads.
#include "fl_common.h"
#include "fl_bf16.h"
#include "fl_image.h"

#define FL_SERVER_THREADS 64

template <int KIND>
__device__ __forceinline__ void server_elem(const FLServer& p, bool real, float x, float& a, float& m, float& v) {
    if (!real) return;
    const float d = __fsub_rn(a, x);
    if (KIND == FL_SERVER_SGD) {
        m = __fmaf_rn(p.b1, m, d);
        a = __fmaf_rn(p.lr, m, x);
        return;
    }
    m = __fmaf_rn(p.b1, m, __fmul_rn(p.omb1, d));
    if (KIND == FL_SERVER_ADAGRAD) {
        v = __fmaf_rn(d, d, v);
    } else {
        const float d2 = __fmul_rn(d, d);
        const float w = __fmul_rn(p.omb2, d2);
        if (KIND == FL_SERVER_ADAM) {
            v = __fmaf_rn(p.b2, v, w);
        } else {
            const float t = __fsub_rn(v, d2);
            v = t > 0.f ? __fsub_rn(v, w) : (t < 0.f ? __fadd_rn(v, w) : v);
        }
    }
    a = __fmaf_rn(p.lr, __fdiv_rn(m, __fadd_rn(__fsqrt_rn(v), p.tau)), x);
}

template <int KIND>
__device__ __forceinline__ void server_quad(const FLServer& p, bool r0, bool r1, bool r2, bool r3, const float4& x,
                                            float4& a, float4& m, float4& v) {
    server_elem<KIND>(p, r0, x.x, a.x, m.x, v.x);
    server_elem<KIND>(p, r1, x.y, a.y, m.y, v.y);
    server_elem<KIND>(p, r2, x.z, a.z, m.z, v.z);
    server_elem<KIND>(p, r3, x.w, a.w, m.w, v.w);
}

// fp32 mode: float4 i of the image.  Its layer by compile-time-indexed selects; a float4 lies in one
// row and one 4-float swizzle chunk (fl_ldw and the chunk swizzle are multiples of 4).
template <int KIND>
__global__ void __launch_bounds__(FL_SERVER_THREADS)
fl_server_kernel(MLPDesc d, FLServer p, const float* __restrict__ xg, float* __restrict__ ag,
                 const FLState* __restrict__ st) {
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;
    const int i = blockIdx.x * FL_SERVER_THREADS + threadIdx.x;
    if (i >= (d.Pimg >> 2)) return;
    const float4 x = reinterpret_cast<const float4*>(xg)[i];
    float4 a = reinterpret_cast<const float4*>(ag)[i];
    float4 m = reinterpret_cast<const float4*>(p.m)[i];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (KIND != FL_SERVER_SGD) v = reinterpret_cast<const float4*>(p.v)[i];
    const int lim = fl_image_lim(d, 4 * i);  // elements j < lim of the float4 are real parameters
    server_quad<KIND>(p, 0 < lim, 1 < lim, 2 < lim, 3 < lim, x, a, m, v);
    reinterpret_cast<float4*>(ag)[i] = a;
    reinterpret_cast<float4*>(p.m)[i] = m;
    if (KIND != FL_SERVER_SGD) reinterpret_cast<float4*>(p.v)[i] = v;
}

// bf16 mode: work item id of the packed parameter region (W items of 8 elements, then bias slots).
template <int KIND>
__global__ void __launch_bounds__(FL_SERVER_THREADS)
fl_server_pack_kernel(MLPDesc d, MLPDescB e, FLServer p, const float* __restrict__ xg, float* __restrict__ ag,
                      const FLState* __restrict__ st, char* __restrict__ out) {
    int r;
    const bool step = fl_round_gate(st, p.max_rounds, r);
    const int id = blockIdx.x * FL_SERVER_THREADS + threadIdx.x;
    const int total = e.item_base[d.L];
    if (id < total) {
        int l = 0;
#pragma unroll
        for (int q = 1; q < FL_MAX_LAYERS; ++q) l += (q < d.L && id >= e.item_base[q]) ? 1 : 0;
        const int loc = id - e.item_base[l];
        const int nch = e.kp[l] >> 3;
        const int n = loc / nch, ch = loc - n * nch;
        const int K = d.dim[l], N = d.dim[l + 1];
        const int K16 = (K + 15) & ~15, N16 = (N + 15) & ~15;
        const bool ok = n < N16 && 8 * ch < K16;
        uint4 hi = make_uint4(0u, 0u, 0u, 0u), lo = make_uint4(0u, 0u, 0u, 0u);
        if (ok) {
            const int o = (d.iw_off[l] + n * fl_ldw(K) + 8 * ch) >> 2;  // float4 index of the item's first half
            float4 a0 = reinterpret_cast<const float4*>(ag)[o], a1 = reinterpret_cast<const float4*>(ag)[o + 1];
            if (step) {
                const float4 x0 = reinterpret_cast<const float4*>(xg)[o], x1 = reinterpret_cast<const float4*>(xg)[o + 1];
                float4 m0 = reinterpret_cast<const float4*>(p.m)[o], m1 = reinterpret_cast<const float4*>(p.m)[o + 1];
                float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
                if (KIND != FL_SERVER_SGD) {
                    v0 = reinterpret_cast<const float4*>(p.v)[o];
                    v1 = reinterpret_cast<const float4*>(p.v)[o + 1];
                }
                // physical column 8 ch + j holds logical column (8 ch + j) ^ fl_swz(n)
                const int s = fl_swz(n);
                const int lim0 = n < N ? K - ((8 * ch) ^ s) : 0, lim1 = n < N ? K - ((8 * ch + 4) ^ s) : 0;
                server_quad<KIND>(p, 0 < lim0, 1 < lim0, 2 < lim0, 3 < lim0, x0, a0, m0, v0);
                server_quad<KIND>(p, 0 < lim1, 1 < lim1, 2 < lim1, 3 < lim1, x1, a1, m1, v1);
                reinterpret_cast<float4*>(ag)[o] = a0;
                reinterpret_cast<float4*>(ag)[o + 1] = a1;
                reinterpret_cast<float4*>(p.m)[o] = m0;
                reinterpret_cast<float4*>(p.m)[o + 1] = m1;
                if (KIND != FL_SERVER_SGD) {
                    reinterpret_cast<float4*>(p.v)[o] = v0;
                    reinterpret_cast<float4*>(p.v)[o + 1] = v1;
                }
            }
            const bool sw = fl_swz(n) != 0;  // the image's swizzled rows hold the two halves swapped
            const float4 p0 = sw ? a1 : a0, p1 = sw ? a0 : a1;
            hi = make_uint4(pack_bf16x2(p0.x, p0.y), pack_bf16x2(p0.z, p0.w), pack_bf16x2(p1.x, p1.y),
                            pack_bf16x2(p1.z, p1.w));
            lo = make_uint4(pack_lo_bf16x2(p0.x, p0.y), pack_lo_bf16x2(p0.z, p0.w), pack_lo_bf16x2(p1.x, p1.y),
                            pack_lo_bf16x2(p1.z, p1.w));
        }
        char* dst = out + e.w_off[l] - e.param_off + fl_wrow(n, e.ldw[l], e.wgap) + 16 * (ch ^ fl_wswz(n, e.wxor));
        *reinterpret_cast<uint4*>(dst) = hi;
        *reinterpret_cast<uint4*>(dst + e.wlo_delta) = lo;
        return;
    }
    int bid = id - total;
    for (int l = 0; l < d.L; ++l) {
        if (bid < e.kp[l + 1]) {
            const int N = d.dim[l + 1], N16 = (N + 15) & ~15;
            float a = 0.f;
            if (bid < N16) {
                const int j = d.ib_off[l] + bid;
                a = ag[j];
                if (step) {
                    float m = p.m[j], v = KIND != FL_SERVER_SGD ? p.v[j] : 0.f;
                    server_elem<KIND>(p, bid < N, xg[j], a, m, v);
                    ag[j] = a;
                    p.m[j] = m;
                    if (KIND != FL_SERVER_SGD) p.v[j] = v;
                }
            }
            reinterpret_cast<float*>(out + e.bias_off[l] - e.param_off)[bid] = a;
            return;
        }
        bid -= e.kp[l + 1];
    }
}

template <int KIND>
static void server_launch(const MLPDesc& d, const FLServer& p, const float* x, float* a, const FLState* st,
                          const MLPDescB* e, char* pk, hipStream_t s) {
    if (e == nullptr) {
        const int n = d.Pimg >> 2;
        hipLaunchKernelGGL(fl_server_kernel<KIND>, dim3((n + FL_SERVER_THREADS - 1) / FL_SERVER_THREADS),
                           dim3(FL_SERVER_THREADS), 0, s, d, p, x, a, st);
    } else {
        int n = e->item_base[d.L];
        for (int l = 0; l < d.L; ++l) n += e->kp[l + 1];
        hipLaunchKernelGGL(fl_server_pack_kernel<KIND>, dim3((n + FL_SERVER_THREADS - 1) / FL_SERVER_THREADS),
                           dim3(FL_SERVER_THREADS), 0, s, d, *e, p, x, a, st, pk);
    }
}

hipError_t fl_launch_server(const MLPDesc& d, const FLServer& p, const float* x, float* a, const FLState* st,
                            const MLPDescB* e, char* pk, hipStream_t s) {
    if ((d.Pimg & 3) != 0 || x == nullptr || a == nullptr || x == a || st == nullptr || p.m == nullptr ||
        (p.kind != FL_SERVER_SGD && p.v == nullptr) || p.max_rounds < 1 || (e == nullptr) != (pk == nullptr))
        return hipErrorInvalidValue;
    switch (p.kind) {
        case FL_SERVER_SGD: server_launch<FL_SERVER_SGD>(d, p, x, a, st, e, pk, s); break;
        case FL_SERVER_ADAGRAD: server_launch<FL_SERVER_ADAGRAD>(d, p, x, a, st, e, pk, s); break;
        case FL_SERVER_ADAM: server_launch<FL_SERVER_ADAM>(d, p, x, a, st, e, pk, s); break;
        case FL_SERVER_YOGI: server_launch<FL_SERVER_YOGI>(d, p, x, a, st, e, pk, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
