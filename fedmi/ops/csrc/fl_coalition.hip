// Coalition utilities for client contribution scores (Shapley values, leave-one-out): before a round's
// aggregation overwrites the K clients' contribution buffers, build the model every coalition of a static mask
// table would have produced alone and score each on the held-out rows -- M models, no per-coalition host launch.
//
// With S_r the round's sampled clients (rtab mask of the round in `st`), v_i client i's contribution image
// (already scaled by its FedAvg weight w_i = cw[r][i]), x the image the round trained from and, for coalition
// m, T' = masks[m] & S_r:
//
//   num[p] = left fold from +0, in client order, over i in T' of v_i[p]      den = the same fold of w_i
//   model[p] = div(num[p], den);   T' empty: x[p], selected (never 0 / 0);   image padding: exact 0
//
// Members are selected in, never multiplied by 0: a NaN in a non-member stays out.  Every operation is one
// round-to-nearest fp32 operation (the kernels below the include are compiled with contraction off and the file
// without the packed fp32 forms), so fedmi/fl/contribution.py coalition_images_model is the build's host model
// bit for bit.  This is the FedAvg the coalition would have produced; no server-optimizer step is applied.
//
//   fl_coalition_build_kernel<KB, VEC> : one thread owns one float4 of the image (K <= 8) or one float (wider
//       buckets, as fl_robust: 64 x 4 source registers would not fit).  It loads its position from all K sources
//       and from x -- every load issued before the first use -- and then walks the M masks in tiles of
//       FL_COALITION_THREADS: per tile, thread t folds the weight row into den of mask m0 + t and leaves it with
//       the effective mask in LDS (den and T' depend on the mask only: computed once per workgroup per mask, by
//       256 lanes at once instead of wave 0 alone); then every thread walks the tile -- the mask read back
//       wave-uniform, the select-fold of its K registers, one division, one plain vector store to
//       scratch[m][Pimg].  Sources are read once however large M is.  No atomics, no grid barrier.
//   fl_coalition_rows_kernel<RT> : the held-out row kernel's forward (stage_image, stage_rows, forward_block of
//       fl_kernels.hip) on a grid of (coalition m, row slice s).  A workgroup stages ITS coalition's image into
//       LDS once and then walks the row blocks [s n_blk / S, (s + 1) n_blk / S) of its slice in a plain loop
//       (the next block's rows are not staged under the current head: the activation window holds one block):
//       the image stage, 45 KB at the reference shape, is paid per workgroup, not per R rows.  S is
//       fl_coalition_slices(M, n_blk), a function of the shapes alone.  One thread adds a block's losses in row
//       order from +0, and the block sums in block order from +0; the correct rows are counted by ballot.  One
//       partial {correct, loss sum} per workgroup, plain stores.
//   fl_coalition_fold_kernel : one thread per coalition adds its S partials in slice order from +0 and writes
//       row r of the device history.
//
// All three are gated by fl_round_gate on the state of the round's output parity and take no per-round host
// argument: they capture into graphs, and a round that is not live writes nothing.
#define FL_FP32_DEVICE_ONLY
#include "fl_kernels.hip"
#include "fl_image.h"

#pragma clang fp contract(off)

template <int KB, int VEC>
__global__ void __launch_bounds__(FL_COALITION_THREADS)
fl_coalition_build_kernel(MLPDesc d, FLCoalition p, const float* const* __restrict__ src, const float* __restrict__ x,
                          const FLState* __restrict__ st) {
    constexpr int T = FL_COALITION_THREADS;
    __shared__ float den_s[T];
    __shared__ uint32_t eff_s[2][T];
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;   // (uniform)
    const uint64_t sampled = fl_round_mask(p.rtab, r, p.K);
    const int idx = VEC * (blockIdx.x * T + threadIdx.x);
    const bool in = idx < d.Pimg;
    const int li = in ? idx : d.Pimg - VEC;   // (threads past the image stay for the tiles' barriers)
    float v[KB][VEC], xv[VEC];
    fl_src_load<KB, VEC>(src, p.K, 0, li, v);
    if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(x + li);
        xv[0] = q.x; xv[1] = q.y; xv[2] = q.z; xv[3] = q.w;
    } else {
        xv[0] = x[li];
    }
    // real parameters among this thread's elements: e < lim
    const int lim = VEC == 4 ? fl_image_lim(d, li) : ((li & 3) < fl_image_lim(d, li & ~3) ? 1 : 0);
    const float* cw = p.cw + (size_t)r * p.K;
    for (int m0 = 0; m0 < p.M; m0 += T) {
        // den and the effective mask of coalition m0 + t: once per workgroup per mask
        const int mm = m0 + (int)threadIdx.x;
        const uint64_t mine = mm < p.M ? (p.masks[mm] & sampled) : 0;
        float den = 0.f;
        for (int i = 0; i < p.K; ++i) den = ((mine >> i) & 1) ? den + cw[i] : den;
        den_s[threadIdx.x] = den;
        eff_s[0][threadIdx.x] = (uint32_t)mine;
        eff_s[1][threadIdx.x] = (uint32_t)(mine >> 32);
        __syncthreads();
        const int mt = p.M - m0 < T ? p.M - m0 : T;
        for (int j = 0; j < mt; ++j) {
            const uint32_t lo = __builtin_amdgcn_readfirstlane(eff_s[0][j]);
            const uint32_t hi = KB > 32 ? __builtin_amdgcn_readfirstlane(eff_s[1][j]) : 0u;
            const float dn = den_s[j];
            float out[VEC];
            if ((lo | hi) == 0) {   // (uniform) nobody: the image the round trained from
#pragma unroll
                for (int e = 0; e < VEC; ++e) out[e] = xv[e];
            } else {
                float num[VEC];
#pragma unroll
                for (int e = 0; e < VEC; ++e) num[e] = 0.f;
#pragma unroll
                for (int i = 0; i < KB; ++i) {
                    const bool on = (((i < 32 ? lo : hi) >> (i & 31)) & 1u) != 0;   // (bits >= K are cut by fl_round_mask)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) num[e] = on ? num[e] + v[i][e] : num[e];
                }
#pragma unroll
                for (int e = 0; e < VEC; ++e) out[e] = __fdiv_rn(num[e], dn);
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) out[e] = e < lim ? out[e] : 0.f;
            if (in) {
                float* o = p.scratch + (size_t)(m0 + j) * d.Pimg + idx;
                if constexpr (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(out[0], out[1], out[2], out[3]);
                else *o = out[0];
            }
        }
        __syncthreads();   // (the next tile rewrites den_s / eff_s)
    }
}

template <int RT>
__global__ void __launch_bounds__(FL_THREADS)
fl_coalition_rows_kernel(MLPDesc d, FLCoalition p, int n_blk, int2* __restrict__ part, const FLState* __restrict__ st) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ __attribute__((aligned(16))) float loss_s[32];
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;
    constexpr int R = RT * 16;
    const int m = blockIdx.x, s = blockIdx.y, S = gridDim.y;
    const int b0 = (int)((long long)s * n_blk / S), b1 = (int)((long long)(s + 1) * n_blk / S);
    const int C = d.dim[d.L];
    float* acts = lds;
    float* li = lds + d.img_lds;
    stage_image(d, p.scratch + (size_t)m * d.Pimg, li);   // once per workgroup, whatever the slice's length
    float total = 0.f;   // (thread 0's)
    int correct = 0;
    for (int b = b0; b < b1; ++b) {
        const int row0 = b * R;
        const int ylab = threadIdx.x < R ? p.y[min(row0 + (int)threadIdx.x, p.n - 1)] : 0;
        stage_rows<RT>(p.X, p.n, d.dim[0], row0, acts + d.act_off[0], d.ld[0]);
        lds_barrier();
        forward_block<RT>(d, acts, li);
        bool hit = false;
        if (threadIdx.x < R) {
            const int rr = threadIdx.x, row = row0 + rr;
            float loss = 0.f;
            if (row < p.n && (unsigned)ylab < (unsigned)C) {
                const float* zr = acts + d.act_off[d.L] + rr * d.ld[d.L];
                const int sr = fl_swz(rr);
                int best = 0;
                float bv = zr[sr];
                for (int k = 1; k < C; ++k)
                    if (zr[k ^ sr] > bv) { bv = zr[k ^ sr]; best = k; }
                float se = 0.f;
                for (int k = 0; k < C; ++k) se = __fadd_rn(se, expf(__fsub_rn(zr[k ^ sr], bv)));
                loss = __fsub_rn(__fadd_rn(bv, logf(se)), zr[ylab ^ sr]);
                hit = best == ylab;
            }
            loss_s[rr] = loss;
        }
        if (threadIdx.x < 64) {   // (the block's R <= 32 rows sit in the first wave)
            const uint64_t h = __ballot(hit);
            if (threadIdx.x == 0) correct += __popcll(h);
        }
        lds_barrier();
        if (threadIdx.x == 0) {
            float bs = 0.f;   // the block's rows from the first to the last, then the blocks in order
#pragma unroll
            for (int q = 0; q < R; ++q) bs = __fadd_rn(bs, loss_s[q]);
            total = __fadd_rn(total, bs);
        }
    }
    if (threadIdx.x == 0) part[(size_t)m * S + s] = make_int2(correct, __float_as_int(total));
}

__global__ void __launch_bounds__(FL_COALITION_THREADS)
fl_coalition_fold_kernel(FLCoalition p, int S, const int2* __restrict__ part, const FLState* __restrict__ st) {
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;
    const int m = blockIdx.x * FL_COALITION_THREADS + threadIdx.x;
    if (m >= p.M) return;
    float sum = 0.f;
    int correct = 0;
    for (int s = 0; s < S; ++s) {
        const int2 q = part[(size_t)m * S + s];
        correct += q.x;
        sum = __fadd_rn(sum, __int_as_float(q.y));
    }
    p.hist_loss[(size_t)r * p.M + m] = sum;
    p.hist_correct[(size_t)r * p.M + m] = correct;
}

hipError_t fl_set_lds_limit_coalition(size_t bytes) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fl_coalition_rows_kernel<1>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(fl_coalition_rows_kernel<2>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e;
}

static bool coalition_args_ok(const MLPDesc& d, const FLCoalition& p) {
    return (d.Pimg & 3) == 0 && d.Pimg >= 4 && p.K >= 1 && p.K <= FL_COALITION_MAX_K && p.M >= 1 &&
           p.M <= FL_COALITION_MAX_M && p.max_rounds >= 1 && p.scratch != nullptr;
}

template <int KB, int VEC>
static void coalition_build_launch(const MLPDesc& d, const FLCoalition& p, const float* const* src, const float* x,
                                   const FLState* st, hipStream_t s) {
    const int units = d.Pimg / VEC;
    hipLaunchKernelGGL((fl_coalition_build_kernel<KB, VEC>), dim3((units + FL_COALITION_THREADS - 1) / FL_COALITION_THREADS),
                       dim3(FL_COALITION_THREADS), 0, s, d, p, src, x, st);
}

hipError_t fl_launch_coalition_build(const MLPDesc& d, const FLCoalition& p, const float* const* src, const float* x,
                                     const FLState* st, hipStream_t s) {
    if (!coalition_args_ok(d, p) || src == nullptr || x == nullptr || st == nullptr || p.rtab == nullptr ||
        p.cw == nullptr || p.masks == nullptr)
        return hipErrorInvalidValue;
    if (p.K <= 4) coalition_build_launch<4, 4>(d, p, src, x, st, s);
    else if (p.K <= 8) coalition_build_launch<8, 4>(d, p, src, x, st, s);
    else if (p.K <= 16) coalition_build_launch<16, 1>(d, p, src, x, st, s);
    else if (p.K <= 32) coalition_build_launch<32, 1>(d, p, src, x, st, s);
    else coalition_build_launch<64, 1>(d, p, src, x, st, s);
    return hipGetLastError();
}

hipError_t fl_launch_coalition_score(const MLPDesc& d, int R, const FLCoalition& p, int slices, const FLState* st,
                                     hipStream_t s) {
    const size_t lds_bytes = (size_t)d.lds_floats * sizeof(float);
    if (!coalition_args_ok(d, p) || (R != 16 && R != 32) || p.n < 1 || p.n > FL_HELDOUT_MAX_ROWS || d.L < 1 ||
        d.L > FL_MAX_LAYERS || d.dim[d.L] < 1 || d.dim[d.L] > FL_MAX_CLASSES || lds_bytes > FL_LDS_DYNAMIC_MAX ||
        p.X == nullptr || p.y == nullptr || p.hist_loss == nullptr || p.hist_correct == nullptr || st == nullptr)
        return hipErrorInvalidValue;
    const int n_blk = (p.n + R - 1) / R;
    const int S = slices == 0 ? fl_coalition_slices(p.M, n_blk) : slices;
    if (S < 1 || S > n_blk || S > 65535) return hipErrorInvalidValue;
    int2* part = reinterpret_cast<int2*>(p.scratch + (size_t)p.M * d.Pimg);
    if (R == 16)
        hipLaunchKernelGGL(fl_coalition_rows_kernel<1>, dim3(p.M, S), dim3(FL_THREADS), lds_bytes, s, d, p, n_blk, part, st);
    else
        hipLaunchKernelGGL(fl_coalition_rows_kernel<2>, dim3(p.M, S), dim3(FL_THREADS), lds_bytes, s, d, p, n_blk, part, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fl_coalition_fold_kernel, dim3((p.M + FL_COALITION_THREADS - 1) / FL_COALITION_THREADS),
                       dim3(FL_COALITION_THREADS), 0, s, p, S, part, st);
    return hipGetLastError();
}
