// Body of the fp32 train kernel (fl_kernels.hip), included verbatim by fl_train_kernel and
// fl_train_batch_kernel (see fl_train_bf16_body.inc) and by fl_train_spec_kernel (fl_train_spec.hip:
// d is a compile-time constant).  In scope: RT, SP (the shape policy, fl_layout.h), d, c, b, pg,
// st_in, st_out, local_step, mode, cm_out, fold_mask.
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ FLState S_sh;
    __shared__ int dgrad_done;  // backward: long-chain dgrad waves finished so far (wgrad_waves_fp32)
    FL_STAMP(0);
    if (b.dbg != nullptr && threadIdx.x == 0) b.dbg[blockIdx.x * 16 + 13] = __builtin_amdgcn_s_memtime();
    int* cm_s = reinterpret_cast<int*>(lds + d.cm_off);
    const int C = d.dim[d.L];
    if (threadIdx.x == 0) dgrad_done = 0;  // (ordered before its first use by the staging barrier)
    if (threadIdx.x < 64) {  // wave 0: round bookkeeping while the other waves stage
        FLState S0 = *st_in;
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
                // fused (fl_common.h): the Adam kernel folds and decides; train tentatively
                S0.live = (!S0.stopped && S0.next_round < c.max_rounds) ? 1 : 0;
            }
        }
        if (threadIdx.x == 0) {
            S_sh = S0;
            cm_s[FL_CM_FLAG] = (local_step == 0 && mode == FL_EVAL_FUSED && S0.next_round > S0.finalized) ? 1 : 0;
        }
    }
    for (int i = threadIdx.x; i < C * C; i += FL_THREADS) cm_s[i] = 0;
    const float* params = (local_step == 0) ? pg : b.local;
    const int R = RT * 16;
    const int row0 = blockIdx.x * R;
    const int L = d.L;
    float* acts = lds;
    float* li = lds + d.img_lds;
    // staging does not depend on the state: it overlaps the finalize above
    // labels are needed only after the forward pass: issue the load now
    const int ylab = (threadIdx.x < R) ? b.y[min(row0 + (int)threadIdx.x, c.n_rows - 1)] : 0;
    stage_image<SP>(d, params, li);
    stage_rows<RT>(b.X, c.n_rows, d.dim[0], row0, acts + d.act_off[0], d.ld[0]);
    lds_barrier();
    FL_STAMP(1);
    if (!S_sh.live) return;
    float* slab = b.slab + (size_t)blockIdx.x * c.slab_stride;
    forward_block<RT, SP>(d, acts, li, b.dbg);
    FL_STAMP(2);
    if (b.dbg != nullptr && threadIdx.x == 0) b.dbg[blockIdx.x * 16 + 14] = __builtin_amdgcn_s_memtime();

    // softmax cross-entropy (mean over the local shard): dZ = (softmax - onehot) / n.
    // Fused evaluation: the same logits score the previous round's model (argmax).
    float* z = acts + d.act_off[L];
    const int ldz = d.ld[L];
    const bool score = cm_s[FL_CM_FLAG] != 0;
    float lossv = 0.f;
    if (threadIdx.x < R) {
        const int r = threadIdx.x, row = row0 + r;
        float* zr = z + r * ldz;
        const int sr = fl_swz(r);  // logit k of row r at column k ^ sr (fl_kernels.hip LDS swizzle)
        if (row < c.n_rows && C == 2) {
            // two classes (the reference's income label): both logits read once, the general
            // loop's arithmetic in the same order (bit-identical)
            const int y = ylab;
            const float z0 = zr[sr], z1 = zr[1 ^ sr];
            const float mx = fmaxf(z0, z1);
            if (score) atomicAdd(&cm_s[y * 2 + (z1 > z0 ? 1 : 0)], 1);
            const float e0 = expf(z0 - mx), e1 = expf(z1 - mx);
            const float se = (0.f + e0) + e1;
            lossv = (mx + logf(se) - (y ? z1 : z0)) * c.inv_n;
            zr[sr] = (e0 / se - (y == 0 ? 1.f : 0.f)) * c.inv_n;
            zr[1 ^ sr] = (e1 / se - (y == 1 ? 1.f : 0.f)) * c.inv_n;
        } else if (row < c.n_rows) {
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
            const float lse = mx + logf(se);
            lossv = (lse - zr[y ^ sr]) * c.inv_n;
            for (int k = 0; k < C; ++k) {
                const float p = expf(zr[k ^ sr] - mx) / se;
                zr[k ^ sr] = (p - (k == y ? 1.f : 0.f)) * c.inv_n;
            }
        } else {
            for (int k = 0; k < C; ++k) zr[k ^ sr] = 0.f;
        }
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

    // backward, top layer first, ONE phase per layer: wgrad_l (reads dZ_{l+1}, act_l) and
    // dgrad_l (reads dZ_{l+1}, W_l, act_l; writes dH_l into its own buffer) are independent.
    // A layer whose dgrad runs on waves of its own (long chains, wgrad_waves_fp32) ends without a
    // barrier: its dgrad waves count themselves done in LDS and every wave starts the next layer
    // once all of them are -- the next phase reads dH_l (the dgrad's output) and act_{l-1}, while
    // this phase's wgrad tiles read only dZ_{l+1} and act_l and write the slab, and the next phase
    // writes only dH_{l-1} and the slab -- so the wgrad tiles overlap the next layer; that layer's
    // tiles go to the dgrad waves first (from the top), which are free earliest.
    int dgrad_target = 0;
    bool from_top = false;
#pragma unroll SP::kStatic ? FL_MAX_LAYERS : 1  // static shape: one copy per layer, constants throughout
    for (int l = L - 1; l >= 0; --l) {
        const float* dz = (l == L - 1) ? acts + d.act_off[L] : acts + d.dlt_off[l + 1];
        const float* act = acts + d.act_off[l];
        const int nw = wgrad_waves_fp32(d.dim[l], d.dim[l + 1], l);
        // (from the top only when every wave takes tiles: with nw < FL_WAVES this layer's own dgrad
        // chains hold the top waves, so its tiles stay on waves [0, nw) -- ADVICE r4)
        wgrad_layer<RT>(d.dim[l], d.dim[l + 1], dz, d.ld[l + 1], act, d.ld[l], slab + d.w_off[l],
                        slab + d.b_off[l], nw, from_top && nw == FL_WAVES);
#ifdef FL_STAMP_FINE  // profiling builds only (tools/probes/stamps_fine.py fp32): wgrad / dgrad split
        if (l == L - 2) FL_STAMP(7);
        if (l == L - 2 && b.dbg != nullptr && threadIdx.x == 64 * (FL_WAVES - 1))  // last wave: dgrad start
            b.dbg[blockIdx.x * 16 + 11] = __builtin_amdgcn_s_memrealtime();
#endif
        if (l > 0)
            dgrad_layer<RT, SP::kStatic>(li + d.iw_off[l], fl_ldw(d.dim[l]), d.dim[l], d.dim[l + 1], dz, d.ld[l + 1], act,
                            d.ld[l], acts + d.dlt_off[l]);
#ifdef FL_STAMP_FINE
        if (l == L - 2 && b.dbg != nullptr && threadIdx.x == 64 * (FL_WAVES - 1))  // last wave: dgrad end
            b.dbg[blockIdx.x * 16 + 12] = __builtin_amdgcn_s_memrealtime();
#endif
        if (nw < FL_WAVES && l > 0) {
            dgrad_target += FL_WAVES - nw;
            if ((int)(threadIdx.x >> 6) >= nw) lds_count_arrive(&dgrad_done);
            lds_count_wait(&dgrad_done, dgrad_target);
            from_top = true;
        } else {
            lds_barrier();
            from_top = false;
        }
        FL_STAMP(4 + (L - 1 - l));
    }
    FL_STAMP(15);
