// Low-rank update compression (PowerSGD, Vogels et al. 2019): one warm-started rank-r power iteration per
// weight matrix, in the compression slot behind the round's last Adam kernel, with the geometry, the gate
// and the parity-buffered residual of fl_compress.hip.  With x the image the round trained from, e the
// client's residual, w its FedAvg weight (rtab), on the P real parameters:
//
//   u  = (local - x) + e
//   c  = C(u)                                   e' = error_feedback ? u - c : 0
//   contribution = w * (x + c)                  image padding is never read or written
//
// C works layer by layer.  Biases travel raw (c = u, e' = 0), and so does a weight matrix whose factors
// would cost as much as the matrix, r (N + K) >= N K.  A compressed layer's block of u is the row-major
// M [N][K] (N out, K in), Q [K][r] its state:
//
//   P = M Q;  P's columns orthonormalised by modified Gram-Schmidt in column order (a column of squared
//   norm 0 becomes the zero column);  Q' = M^T P;  c = P Q'^T;  Q <- Q'
//
// If one of the r squared norms is not finite the layer travels raw this round and keeps its Q.
//
// Rounding and order (fedmi/fl/compress.py lowrank_torch is the bit-exact host model).  Every operation
// is one fp32 rounding: products and sums are separate (this file is compiled with contraction off and
// without the packed fp32 forms, fedmi/ops/build.py), sqrtf is the correctly rounded root, one division
// per element of P.  The dot products of M Q (over k), M^T P (over n) and P Q'^T (over j) run in ascending
// contraction index from +0.  A Gram-Schmidt dot over N is summed as one wave does: lane t adds entries
// t, t + 64, ... in turn from +0, then the xor tree 32 .. 1.  The statistic sqrt(sum (u - c)^2) /
// sqrt(sum u^2) (0 where u = 0) takes both sums over all P entries in block_sum_ordered's order.
// No order depends on the grid or on the workgroup.
//
// No cross-workgroup dependency: every workgroup recomputes all factors from the L2-resident inputs, so Q
// is double-buffered by round parity exactly as the residual is (round r reads half r & 1 and writes half
// (r + 1) & 1; an unsampled client carries both over).  Inside a workgroup of 1024 threads:
//   1. u of all P parameters into LDS in dense order (clamped loads four at a time: 12 global loads in
//      flight per thread), Q into LDS.
//   2. all compressed layers' P entries at once, one (layer, n, j) item per thread, j fastest.
//   3. Gram-Schmidt, one wave per compressed layer, all layers at once.  Lane t owns rows t, t + 64, ... of
//      its layer's P: every LDS word has one reader and writer, lanes meet in the shuffles only.
//   4. all layers' Q' entries at once, one (layer, j, k) item per thread, k fastest.
//   5. the workgroup's quads of dense parameters: c from the P row and the Q' row, both r-contiguous in LDS
//      (ds_read_b128 / b64 for even r), then contribution and residual half; the Q half, one owner per
//      entry over the grid; the statistic in workgroup 0.
// LDS: 4 P + 4 r (sum N + 2 sum K) bytes over the compressed layers, 45 KB + 6 KB at 14-50-200-2, r = 4.
//
// Bank conflicts (64 banks x 4 B).  Step 4 reads M[n][k] with lanes along k: consecutive words, consecutive
// banks, and P[n][j] is one word per j: a broadcast.  Step 2 reads M[n][k] with 64 / r rows per wave (the r
// lanes of a row read one word): rows are K words apart, so two rows collide when K (n1 - n2) = 0 mod 64.
// K = 14 and K = 50 are 2 x odd: rows 32 apart collide, a wave holds at most 64 / r <= 32 consecutive rows
// for r >= 2 -- conflict free -- and r = 1 is 2-way.  Odd K (17) is conflict free at every r; a K that is
// a multiple of 64 would be 64 / r-way and wants a padded row, which no shape here needs.  Step 3's column
// walks are r words apart (r-way for r = 2, 4, 8): 4 words per lane and dot, off the long chains.
//
// v_mfma_f32_16x16x4f32 is deliberately not used: r <= 8 fills at most half of a 16-wide tile, the whole
// step is about 6 r P flops and latency-bound, and the instruction's internal summation order cannot be
// reproduced by the numpy model the tests of this family rest on.
#include "fl_common.h"
#include "fl_device.h"
#include "fl_image.h"

#define FL_LR_THREADS 1024

// One rounding per operation whatever the flags (as fl_geomed.hip's and fl_attack.hip's helpers): with
// contraction off a product that feeds a sum stays a v_mul_f32 and a v_add_f32.
#pragma clang fp contract(off)
__device__ __forceinline__ float lr_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float lr_add(float a, float b) { return a + b; }
__device__ __forceinline__ float lr_sub(float a, float b) { return a - b; }

// Layer l's shape and offsets.  The kernel keeps the table in LDS (filled from the kernel arguments with
// compile-time indices), so a lookup by a run-time layer is one broadcast LDS read, not a private array.
struct LrLayer {
    int K, N, wo, po, qo;  // in, out, dense offset of W, LDS offset of P [N][r], offset of Q [K][r]
};
__device__ __forceinline__ void lr_layers(const MLPDesc& d, const FLLowRank& p, LrLayer* lay) {
#pragma unroll
    for (int t = 0; t < FL_MAX_LAYERS; ++t) lay[t] = {d.dim[t], d.dim[t + 1], d.w_off[t], p.p_off[t], p.q_off[t]};
}
// The layer that owns item i of a prefix-summed item range (off[t] = items of the compressed layers before
// t; a layer without items shares its offset with the next one, which then wins).
template <bool OF_Q>
__device__ __forceinline__ int lr_owner(const MLPDesc& d, const FLLowRank& p, int i) {
    int l = 0;
#pragma unroll
    for (int t = 1; t < FL_MAX_LAYERS; ++t)
        if (t < d.L && i >= (OF_Q ? p.q_off[t] : p.p_off[t])) l = t;
    return l;
}

// Dense index -> image position (as fl_image_index), layer, row and column (k < 0: a bias).
struct LrAt {
    int j, l, n, k;
};
__device__ __forceinline__ LrAt lr_at(const MLPDesc& d, int di) {
    int l = 0, K = d.dim[0], wo = d.w_off[0], bo = d.b_off[0], iwo = d.iw_off[0], ibo = d.ib_off[0];
#pragma unroll
    for (int t = 1; t < FL_MAX_LAYERS; ++t)
        if (t < d.L && di >= d.w_off[t]) {
            l = t; K = d.dim[t]; wo = d.w_off[t]; bo = d.b_off[t]; iwo = d.iw_off[t]; ibo = d.ib_off[t];
        }
    if (di >= bo) return {ibo + (di - bo), l, di - bo, -1};
    const int q = di - wo;
    const int n = q / K, k = q - n * K;
    return {iwo + n * fl_ldw(K) + (k ^ fl_swz(n)), l, n, k};
}

// R consecutive LDS floats at an R-aligned offset of a 16-byte aligned array: vector reads for even R.
template <int R>
__device__ __forceinline__ void lr_row(const float* s, float (&v)[R]) {
    if constexpr (R % 4 == 0) {
#pragma unroll
        for (int i = 0; i < R; i += 4) {
            const float4 t = *reinterpret_cast<const float4*>(s + i);
            v[i] = t.x; v[i + 1] = t.y; v[i + 2] = t.z; v[i + 3] = t.w;
        }
    } else if constexpr (R % 2 == 0) {
#pragma unroll
        for (int i = 0; i < R; i += 2) {
            const float2 t = *reinterpret_cast<const float2*>(s + i);
            v[i] = t.x; v[i + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < R; ++i) v[i] = s[i];
    }
}

// c of the dense entry at `a` with update u; `raw`: the entry travels as it is (bias, uncompressed layer,
// layer with a squared norm that is not finite).
template <int R>
__device__ __forceinline__ float lr_c(const LrLayer* lay, const FLLowRank& p, const LrAt& a, float u, const float* ps,
                                      const float* qn, const int* bad, bool& raw) {
    raw = a.k < 0 || !((p.comp >> a.l) & 1) || bad[a.l] != 0;
    if (raw) return u;
    const LrLayer y = lay[a.l];
    float pr[R], qr[R];
    lr_row<R>(ps + y.po + a.n * R, pr);
    lr_row<R>(qn + y.qo + a.k * R, qr);
    float c = 0.f;
#pragma unroll
    for (int j = 0; j < R; ++j) c = lr_add(c, lr_mul(pr[j], qr[j]));
    return c;
}

template <int R>
__global__ void __launch_bounds__(FL_LR_THREADS)
fl_lowrank_kernel(MLPDesc d, FLLowRank p, const float* __restrict__ local, const float* __restrict__ pg,
                  float* __restrict__ comm, const FLState* __restrict__ st, const float* __restrict__ rtab) {
    extern __shared__ __attribute__((aligned(16))) float lr_lds[];
    __shared__ int bad[FL_MAX_LAYERS];  // layer l has a squared norm that is not finite
    __shared__ LrLayer lay[FL_MAX_LAYERS];
    __shared__ float wnum[FL_LR_THREADS / 64], wden[FL_LR_THREADS / 64];
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;
    const float w = fl_round_weight(rtab, r);
    const int P = d.P, Qlen = p.Qlen, Plen = p.Plen, tid = threadIdx.x;
    const float* __restrict__ ein = p.residual + (size_t)(r & 1) * d.Pimg;
    float* __restrict__ eout = p.residual + (size_t)((r + 1) & 1) * d.Pimg;
    const float* __restrict__ qin = p.q + (size_t)(r & 1) * Qlen;
    float* __restrict__ qout = p.q + (size_t)((r + 1) & 1) * Qlen;
    const int gt = blockIdx.x * FL_LR_THREADS + tid;  // block of 4 dense parameters
    const int gstride = gridDim.x * FL_LR_THREADS;
    if (w == 0.f) {  // not sampled: the Adam kernel's zeros stay; residual and Q carry over to the next half
        if (gt == 0) p.stat_hist[r] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int di = 4 * gt + k;
            if (di < P) {
                const int j = fl_image_index(d, di);
                eout[j] = ein[j];
            }
        }
        for (int i = gt; i < Qlen; i += gstride) qout[i] = qin[i];
        return;
    }
    float* ubuf = lr_lds;                  // [P] u, dense order (rounded up to whole quads)
    float* ps = ubuf + ((P + 3) & ~3);     // [Plen] P rows, r-contiguous
    float* qn = ps + Plen;                 // [Qlen] Q' rows, r-contiguous
    float* qs = qn + Qlen;                 // [Qlen] Q

    // 1. u and Q into LDS
    const int per = (P + FL_LR_THREADS - 1) / FL_LR_THREADS;  // entries per thread: t, t + 1024, ...
    for (int it = 0; it < per; it += 4) {
        float a[4], x[4], e[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int di = (it + i) * FL_LR_THREADS + tid;
            const int j = fl_image_index(d, di < P ? di : P - 1);
            a[i] = local[j]; x[i] = pg[j]; e[i] = ein[j];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int di = (it + i) * FL_LR_THREADS + tid;
            if (di < P) ubuf[di] = lr_add(lr_sub(a[i], x[i]), e[i]);
        }
    }
    for (int i = tid; i < Qlen; i += FL_LR_THREADS) qs[i] = qin[i];
    if (tid < FL_MAX_LAYERS) bad[tid] = 0;
    if (tid == 64) lr_layers(d, p, lay);
    __syncthreads();

    // 2. P = M Q: item (layer, n, j), j fastest
    for (int i = tid; i < Plen; i += FL_LR_THREADS) {
        const LrLayer y = lay[lr_owner<false>(d, p, i)];
        const int li = i - y.po;
        const int n = li / R, j = li - n * R;
        const float* m = ubuf + y.wo + n * y.K;
        const float* q = qs + y.qo + j;
        float acc = 0.f;
        for (int k = 0; k < y.K; ++k) acc = lr_add(acc, lr_mul(m[k], q[k * R]));
        ps[i] = acc;
    }
    __syncthreads();

    // 3. modified Gram-Schmidt in column order: wave l takes layer l, lane t its rows t, t + 64, ...
    const int wv = tid >> 6, lane = tid & 63;
    if (wv < d.L && ((p.comp >> wv) & 1)) {
        const LrLayer y = lay[wv];
        float* pl = ps + y.po;
        bool notfin = false;
#pragma unroll
        for (int j = 0; j < R; ++j) {
#pragma unroll
            for (int i = 0; i < j; ++i) {
                float acc = 0.f;
                for (int n = lane; n < y.N; n += 64) acc = lr_add(acc, lr_mul(pl[n * R + i], pl[n * R + j]));
                const float dt = wave_sum(acc);
                for (int n = lane; n < y.N; n += 64) pl[n * R + j] = lr_sub(pl[n * R + j], lr_mul(dt, pl[n * R + i]));
            }
            float acc = 0.f;
            for (int n = lane; n < y.N; n += 64) acc = lr_add(acc, lr_mul(pl[n * R + j], pl[n * R + j]));
            const float ss = wave_sum(acc);
            notfin = notfin || (__float_as_uint(ss) & 0x7f800000u) == 0x7f800000u;
            // (sqrtf, not __fsqrt_rn: the correctly rounded root, see fl_compress.hip's qsgd norm)
            const float nrm = sqrtf(ss);
            for (int n = lane; n < y.N; n += 64) pl[n * R + j] = ss == 0.f ? 0.f : __fdiv_rn(pl[n * R + j], nrm);
        }
        if (lane == 0) bad[wv] = notfin ? 1 : 0;
    }
    __syncthreads();

    // 4. Q' = M^T P: item (layer, j, k), k fastest
    for (int i = tid; i < Qlen; i += FL_LR_THREADS) {
        const LrLayer y = lay[lr_owner<true>(d, p, i)];
        const int li = i - y.qo;
        const int j = li / y.K, k = li - j * y.K;
        const float* m = ubuf + y.wo + k;
        const float* pc = ps + y.po + j;
        float acc = 0.f;
        for (int n = 0; n < y.N; ++n) acc = lr_add(acc, lr_mul(m[n * y.K], pc[n * R]));
        qn[y.qo + k * R + j] = acc;
    }
    __syncthreads();

    // 5. the workgroup's quads: contribution and residual half
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int di = 4 * gt + k;
        if (di >= P) break;
        const LrAt a = lr_at(d, di);
        const float u = ubuf[di];
        bool raw;
        const float c = lr_c<R>(lay, p, a, u, ps, qn, bad, raw);
        comm[a.j] = lr_mul(w, lr_add(pg[a.j], c));
        eout[a.j] = p.error_feedback && !raw ? lr_sub(u, c) : 0.f;
    }
    // the Q half, one owner per entry over the grid (a layer that travels raw keeps its Q)
    for (int i = gt; i < Qlen; i += gstride) qout[i] = bad[lr_owner<true>(d, p, i)] ? qs[i] : qn[i];
    // the statistic, workgroup 0: both sums over all P entries in block_sum_ordered's order
    if (blockIdx.x == 0) {
        float an = 0.f, ad = 0.f;
        for (int di = tid; di < P; di += FL_LR_THREADS) {
            const float u = ubuf[di];
            bool raw;
            const float dd = lr_sub(u, lr_c<R>(lay, p, lr_at(d, di), u, ps, qn, bad, raw));
            an = lr_add(an, lr_mul(dd, dd));
            ad = lr_add(ad, lr_mul(u, u));
        }
        const float num = block_sum_ordered<FL_LR_THREADS>(an, wnum);
        const float den = sqrtf(block_sum_ordered<FL_LR_THREADS>(ad, wden));
        if (tid == 0) p.stat_hist[r] = den == 0.f ? 0.f : __fdiv_rn(sqrtf(num), den);
    }
}

// Which layers rank `rank` compresses, the offsets of their Q and P blocks and what a real uplink carries.
hipError_t fl_lowrank_plan(const MLPDesc& d, int rank, FLLowRank& p) {
    if (rank < 1 || rank > FL_LOWRANK_MAX_RANK || d.L < 1 || d.L > FL_MAX_LAYERS) return hipErrorInvalidValue;
    p.rank = rank;
    p.comp = 0;
    p.entries = 0;
    int po = 0, qo = 0;
    for (int l = 0; l <= FL_MAX_LAYERS; ++l) {
        p.p_off[l] = po;
        p.q_off[l] = qo;
        if (l >= d.L) continue;
        const long long K = d.dim[l], N = d.dim[l + 1];
        if (rank * (N + K) < N * K) {
            p.comp |= 1 << l;
            po += rank * (int)N;
            qo += rank * (int)K;
            p.entries += rank * (int)(N + K) + (int)N;
        } else {
            p.entries += (int)(N * K + N);
        }
    }
    p.Plen = po;
    p.Qlen = qo;
    return hipSuccess;
}

static inline size_t lr_lds_bytes(const MLPDesc& d, const FLLowRank& p) {
    return sizeof(float) * ((((size_t)d.P + 3) & ~(size_t)3) + (size_t)p.Plen + 2 * (size_t)p.Qlen);
}

template <int R>
static hipError_t lr_dispatch(int want, bool launch, const MLPDesc& d, const FLLowRank& p, size_t lds, dim3 grid,
                              const float* local, const float* pg, float* comm, const FLState* st, const float* rtab,
                              hipStream_t s) {
    if constexpr (R > FL_LOWRANK_MAX_RANK) {
        return hipErrorInvalidValue;
    } else {
        if (want != R) return lr_dispatch<R + 1>(want, launch, d, p, lds, grid, local, pg, comm, st, rtab, s);
        if (!launch)
            return hipFuncSetAttribute(reinterpret_cast<const void*>(fl_lowrank_kernel<R>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(fl_lowrank_kernel<R>, grid, dim3(FL_LR_THREADS), lds, s, d, p, local, pg, comm, st, rtab);
        return hipGetLastError();
    }
}

static bool lr_args_ok(const MLPDesc& d, const FLLowRank& p) {
    FLLowRank q = p;
    if (d.P < 1 || (d.Pimg & 3) != 0 || fl_lowrank_plan(d, p.rank, q) != hipSuccess) return false;
    for (int l = 0; l <= FL_MAX_LAYERS; ++l)
        if (q.p_off[l] != p.p_off[l] || q.q_off[l] != p.q_off[l]) return false;
    return q.comp == p.comp && q.Plen == p.Plen && q.Qlen == p.Qlen && lr_lds_bytes(d, p) <= (size_t)FL_LDS_DYNAMIC_MAX;
}

// Dynamic LDS of the kernel for this model and rank; call once before the first launch (the engine's
// constructor does), not inside a stream capture.
hipError_t fl_set_lds_limit_lowrank(const MLPDesc& d, const FLLowRank& p) {
    if (!lr_args_ok(d, p)) return hipErrorInvalidValue;
    return lr_dispatch<1>(p.rank, false, d, p, lr_lds_bytes(d, p), dim3(1), nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr);
}

hipError_t fl_launch_lowrank(const MLPDesc& d, const FLLowRank& p, const float* local, const float* pg, float* comm,
                             const FLState* st, const float* rtab, hipStream_t s) {
    if (!lr_args_ok(d, p) || p.residual == nullptr || p.stat_hist == nullptr || (p.q == nullptr && p.Qlen > 0) ||
        p.max_rounds < 1)
        return hipErrorInvalidValue;
    const int quads = (d.P + 3) / 4;
    const dim3 grid((quads + FL_LR_THREADS - 1) / FL_LR_THREADS);
    return lr_dispatch<1>(p.rank, true, d, p, lr_lds_bytes(d, p), grid, local, pg, comm, st, rtab, s);
}
