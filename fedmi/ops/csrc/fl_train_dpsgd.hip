// Record-level DP-SGD train kernel (Abadi et al. 2016), fp32, in a translation unit of its own so the
// other train kernels' code generation is untouched (the device functions are fl_kernels.hip's, as in
// fl_train_spec.hip).  Every example's whole gradient is clipped to L2 norm C before it enters the
// workgroup's slab row, and one extra workgroup writes a slab row of Gaussian noise z C / n N(0, I),
// which the Adam kernels reduce like any other row: sum_r min(1, C / ||g_r||) g_r / n + z C / n N(0, I).
//
// Per-example norms without per-example gradients ("ghost clipping"): row r's weight gradient in layer l
// is dZ_{l+1}[r] (x) act_l[r] and its bias gradient dZ_{l+1}[r], so
//     ||g_r||^2 = sum_l (1 + ||act_l[r]||^2) ||dZ_{l+1}[r]||^2
// with every operand resident in LDS at once (fl_layout.h: act_off[0..L], dlt_off[1..L-1] are disjoint).
//
// Phases of a row workgroup after the forward pass (the prologue is fl_train_body.inc's: round-state fold
// on wave 0, mode / fold_mask / fused scoring, staging, forward_block, confusion counts, !live return):
//   head   threads < R: dZ_L[r] = softmax - onehot (NOT times 1/n), ||dZ_L[r]||^2, the loss slot as ever
//   A      l = L-1 .. 1: dgrad_l alone -> dlt_off[l].  dgrad_layer keeps ceil(K/16) waves busy (4 of 16
//          for 200 -> 50); the other waves (all of them, after their items, when none is free) take the
//          row norms that are final by then: in the first phase ||act_k[r]||^2 of every layer, in phase l
//          ||dZ_{l+1}[r]||^2.  A last short phase takes ||dZ_1[r]||^2 on all waves.
//          A row norm is one 16-lane group's work: lane j sums the logical columns j, j + 16, ... < dim
//          (fmaf, ascending), then an xor tree over 8, 4, 2, 1 -- one fixed order whichever wave runs it.
//          Only logical columns are read, so no statement about pad columns is needed.
//   f      threads < R: s_r by the formula, layers ascending; f_r = s_r > C^2 ? C / sqrt(s_r) : 1; sqrt(s_r)
//          of the real rows -> row_norm[] (plain stores); f_r / n -> LDS
//   scale  every dZ row times f_r / n IN PLACE in LDS, one sweep over R x (hidden + classes) floats.  In
//          place and not on the A fragment in the tile loop: wgrad_layer and its bias sums are reused as
//          they are, the sweep is one pass over ~9 K floats against RT * 4 extra multiplies in each of the
//          ~190 tiles, and with C above every norm the deltas are bitwise the unclipped kernel's.
//   B      wgrad + bias sums of every layer, all 16 waves on tiles, no barrier between layers (they read
//          LDS and write the slab only)
// The noise workgroup (blockIdx.x == n_slabs - 1) stages nothing: wave 0 reads the round state, then dense
// parameter p takes lane p % 4 of the Box-Muller pairs (fl_dp.hip's) of Philox4x32-10 at counter
// (p / 4, round, rank | local_step << 16, FL_DPSGD_STREAM) under the 64-bit DP-SGD seed; the loss slot and
// the row's padding are 0.  z = 0 takes the same path (sigma = 0).  fedmi/privacy/philox.py dpsgd_normals
// is the host model.  The round index comes from the device state: a replayed graph draws fresh noise.
#define FL_FP32_DEVICE_ONLY
#include "fl_kernels.hip"

// ||buf[r][0 .. dim)||^2 for r in [0, R) -> out[r]; row groups of 4 are dealt to waves [0, nw) (the caller
// passes its wave's index among them).  Logical column k of row r sits at k ^ fl_swz(r).
template <int RT>
__device__ __forceinline__ void row_sqnorms(const float* buf, int ld, int dim, float* out, int w, int nw) {
    const int lane = threadIdx.x & 63, j = lane & 15;
    for (int g = w; g < RT * 4; g += nw) {
        const int r = 4 * g + (lane >> 4);
        const float* row = buf + r * ld;
        const int sw = fl_swz(r);
        float s = 0.f;
        for (int k = j; k < dim; k += 16) {
            const float v = row[k ^ sw];
            s = __fmaf_rn(v, v, s);
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) s = __fadd_rn(s, __shfl_xor(s, off, 64));
        if (j == 0) out[r] = s;
    }
}

template <int RT>
__global__ void __launch_bounds__(FL_THREADS)
fl_train_dpsgd_kernel(MLPDesc d, FLConfig c, FLBuffers b, FLDpSgd p, const float* __restrict__ pg,
                      const FLState* __restrict__ st_in, FLState* __restrict__ st_out, int local_step, int mode,
                      float* __restrict__ cm_out, int fold_mask) {
    using SP = FlShapeDyn;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ FLState S_sh;
    __shared__ int round_sh;                                // the round the launch trains (noise counter)
    __shared__ float na[FL_MAX_LAYERS][32];                 // ||act_l[r]||^2
    __shared__ float nd[FL_MAX_LAYERS + 1][32];             // ||dZ_l[r]||^2, l = 1 .. L
    __shared__ float fac[32];                               // f_r / n
    constexpr int R = RT * 16;
    const int n_blocks = c.n_slabs - 1;                     // row workgroups; the last workgroup is the noise row's
    const bool noise_blk = (int)blockIdx.x == n_blocks;
    if (!noise_blk) FL_STAMP(0);
    int* cm_s = reinterpret_cast<int*>(lds + d.cm_off);
    const int C = d.dim[d.L];
    if (threadIdx.x < 64) {  // wave 0: round bookkeeping while the other waves stage (fl_train_body.inc)
        FLState S0 = *st_in;
        const int rd = local_step == 0 ? S0.next_round : S0.cur_round;
        if (local_step == 0) {
            if (mode == FL_EVAL_CLASSIC) {
                if (blockIdx.x == 0 || fold_may_stop(c, S0))
                    S0 = finalize_state(d, c, b, pg, S0, blockIdx.x == 0, fold_mask);
                if (threadIdx.x == 0) {
                    S0.live = (!S0.stopped && S0.next_round < c.max_rounds) ? 1 : 0;
                    if (S0.live) { S0.cur_round = S0.next_round; S0.next_round += 1; }
                    if (blockIdx.x == 0) *st_out = S0;
                }
            } else if (threadIdx.x == 0) {
                S0.live = (!S0.stopped && S0.next_round < c.max_rounds) ? 1 : 0;
            }
        }
        if (threadIdx.x == 0) {
            S_sh = S0;
            round_sh = rd;
            cm_s[FL_CM_FLAG] = (local_step == 0 && mode == FL_EVAL_FUSED && S0.next_round > S0.finalized) ? 1 : 0;
        }
    }
    if (noise_blk) {
        lds_barrier();
        if (!S_sh.live) return;
        float* row = b.slab + (size_t)n_blocks * c.slab_stride;
        const float sigma = __fmul_rn(__fmul_rn(p.noise, p.clip), c.inv_n);
        const uint32_t rd = (uint32_t)round_sh, who = (uint32_t)c.rank | ((uint32_t)local_step << 16);
        for (int q = threadIdx.x; 4 * q < c.slab_stride; q += FL_THREADS) {
            float nz[4] = {0.f, 0.f, 0.f, 0.f};
            if (4 * q < d.P) {
                const uint4 o = philox4x32_10((uint32_t)q, rd, who, FL_DPSGD_STREAM, p.key0, p.key1);
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
            for (int k = 0; k < 4; ++k) slab_store(&row[4 * q + k], 4 * q + k < d.P ? nz[k] : 0.f);
        }
        return;
    }
    for (int i = threadIdx.x; i < C * C; i += FL_THREADS) cm_s[i] = 0;
    const float* params = (local_step == 0) ? pg : b.local;
    const int row0 = blockIdx.x * R;
    const int L = d.L;
    float* acts = lds;
    float* li = lds + d.img_lds;
    const int ylab = (threadIdx.x < R) ? b.y[min(row0 + (int)threadIdx.x, c.n_rows - 1)] : 0;
    stage_image<SP>(d, params, li);
    stage_rows<RT>(b.X, c.n_rows, d.dim[0], row0, acts + d.act_off[0], d.ld[0]);
    lds_barrier();
    FL_STAMP(1);
    if (!S_sh.live) return;
    float* slab = b.slab + (size_t)blockIdx.x * c.slab_stride;
    forward_block<RT, SP>(d, acts, li, b.dbg);
    FL_STAMP(2);

    // loss head: dZ_L = softmax - onehot (the 1/n rides the clip factor), its squared norm, the loss slot
    float* z = acts + d.act_off[L];
    const int ldz = d.ld[L];
    const bool score = cm_s[FL_CM_FLAG] != 0;
    float lossv = 0.f;
    if (threadIdx.x < R) {
        const int r = threadIdx.x, row = row0 + r;
        float* zr = z + r * ldz;
        const int sr = fl_swz(r);
        float sq = 0.f;
        if (row < c.n_rows) {
            const int y = ylab;
            float mx = zr[sr], bv = zr[sr];
            int best = 0;
            for (int k = 1; k < C; ++k) {
                mx = fmaxf(mx, zr[k ^ sr]);
                if (zr[k ^ sr] > bv) { bv = zr[k ^ sr]; best = k; }  // torch.max(dim=1): first maximum
            }
            if (score) atomicAdd(&cm_s[y * C + best], 1);
            float se = 0.f;
            for (int k = 0; k < C; ++k) se += expf(zr[k ^ sr] - mx);
            lossv = (mx + logf(se) - zr[y ^ sr]) * c.inv_n;
            for (int k = 0; k < C; ++k) {
                const float dz = expf(zr[k ^ sr] - mx) / se - (k == y ? 1.f : 0.f);
                zr[k ^ sr] = dz;
                sq = __fmaf_rn(dz, dz, sq);
            }
        } else {
            for (int k = 0; k < C; ++k) zr[k ^ sr] = 0.f;
        }
        nd[L][r] = sq;
        // (columns [C, roundup16(C)) are zero already: the head's forward writes them)
    }
    if (threadIdx.x < 64) {
        lossv = wave_sum(lossv);
        if (threadIdx.x == 0) slab[d.P] = lossv;  // R <= 64: wave 0 holds every row
    }
    lds_barrier();
    if (score)
        for (int i = threadIdx.x; i < C * C; i += FL_THREADS)
            if (cm_s[i]) atomicAdd(&cm_out[i], (float)cm_s[i]);
    FL_STAMP(3);

    // pass A: the dgrad chain alone; the waves it leaves idle take the row norms that are final
    const int wv = threadIdx.x >> 6;
    bool acts_done = false;
    for (int l = L - 1; l >= 1; --l) {
        const float* dz = (l == L - 1) ? z : acts + d.dlt_off[l + 1];
        dgrad_layer<RT, false>(li + d.iw_off[l], fl_ldw(d.dim[l]), d.dim[l], d.dim[l + 1], dz, d.ld[l + 1],
                               acts + d.act_off[l], d.ld[l], acts + d.dlt_off[l]);
        const int nfree = FL_WAVES - ((d.dim[l] + 15) >> 4);  // dgrad items sit on the top waves
        const int nw = nfree > 0 ? nfree : FL_WAVES;
        if (wv < nw) {
            if (!acts_done)
                for (int k = 0; k < L; ++k) row_sqnorms<RT>(acts + d.act_off[k], d.ld[k], d.dim[k], na[k], wv, nw);
            else
                row_sqnorms<RT>(acts + d.dlt_off[l + 1], d.ld[l + 1], d.dim[l + 1], nd[l + 1], wv, nw);
        }
        acts_done = true;
        lds_barrier();
    }
    if (!acts_done) row_sqnorms<RT>(acts + d.act_off[0], d.ld[0], d.dim[0], na[0], wv, FL_WAVES);  // L == 1
    if (L > 1) row_sqnorms<RT>(acts + d.dlt_off[1], d.ld[1], d.dim[1], nd[1], wv, FL_WAVES);
    lds_barrier();
    FL_STAMP(4);

    // clip factors: one fixed order per row
    if (threadIdx.x < R) {
        const int r = threadIdx.x, row = row0 + r;
        float s = 0.f;
        for (int l = 0; l < L; ++l) s = __fmaf_rn(__fadd_rn(1.f, na[l][r]), nd[l + 1][r], s);
        const float nrm = __fsqrt_rn(s);
        const float f = s > __fmul_rn(p.clip, p.clip) ? __fdiv_rn(p.clip, nrm) : 1.f;
        fac[r] = __fmul_rn(f, c.inv_n);
        if (row < c.n_rows) p.row_norm[row] = nrm;
    }
    lds_barrier();
    // dZ_l[r] *= f_r / n in place (logical columns and the zero pads up to roundup16; the 4 floats behind
    // them are never read)
    for (int l = 1; l <= L; ++l) {
        float* dz = (l == L) ? z : acts + d.dlt_off[l];
        const int w16 = (d.dim[l] + 15) & ~15, ld = d.ld[l];
        for (int e = threadIdx.x; e < R * w16; e += FL_THREADS) {
            const int r = e / w16, k = e - r * w16;
            dz[r * ld + k] = __fmul_rn(dz[r * ld + k], fac[r]);
        }
    }
    lds_barrier();
    FL_STAMP(5);

    // pass B: clipped weight gradients and bias sums, every wave on tiles
    for (int l = L - 1; l >= 0; --l) {
        const float* dz = (l == L - 1) ? z : acts + d.dlt_off[l + 1];
        wgrad_layer<RT>(d.dim[l], d.dim[l + 1], dz, d.ld[l + 1], acts + d.act_off[l], d.ld[l], slab + d.w_off[l],
                        slab + d.b_off[l]);
    }
    FL_STAMP(15);
}

hipError_t fl_launch_train_dpsgd(const MLPDesc& d, const FLConfig& c, const FLBuffers& b, const FLDpSgd& p,
                                 const float* pg, const FLState* si, FLState* so, int ls, hipStream_t s, int mode,
                                 float* cm_out, int fold_mask) {
    if (mode == FL_EVAL_LAGGED || (mode == FL_EVAL_FUSED && cm_out == nullptr)) return hipErrorInvalidValue;
    if (c.slab_f16 || c.n_slabs != (c.n_rows + c.R - 1) / c.R + 1 || (c.slab_stride & 3) != 0 || c.slab_stride <= d.P)
        return hipErrorInvalidValue;  // fp32 rows, one more than the shard has row blocks
    if (!(p.clip > 0.f) || !(p.noise >= 0.f) || p.row_norm == nullptr || ls < 0 || ls > 0xFFFF || c.rank > 0xFFFF)
        return hipErrorInvalidValue;
    const size_t lds = (size_t)d.lds_floats * sizeof(float);
    switch (c.R) {
        case 16:
            hipLaunchKernelGGL(fl_train_dpsgd_kernel<1>, dim3(c.n_slabs), dim3(FL_THREADS), lds, s, d, c, b, p, pg, si,
                               so, ls, mode, cm_out, fold_mask);
            break;
        case 32:
            hipLaunchKernelGGL(fl_train_dpsgd_kernel<2>, dim3(c.n_slabs), dim3(FL_THREADS), lds, s, d, c, b, p, pg, si,
                               so, ls, mode, cm_out, fold_mask);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t fl_set_lds_limit_dpsgd(size_t bytes) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fl_train_dpsgd_kernel<1>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(fl_train_dpsgd_kernel<2>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e;
}
