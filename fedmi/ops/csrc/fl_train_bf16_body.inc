// Body of the bf16 train kernel (fl_kernels_bf16.hip), included verbatim by its two entry
// points -- fl_train_bf16_kernel (arguments = kernel arguments) and fl_train_bf16_batch_kernel
// (the same names bound from the FLTrialDesc table row of blockIdx.y) -- so the single-engine
// kernel compiles to exactly the code it had before trial batches existed -- and by
// fl_train_bf16_spec_kernel (fl_train_bf16_spec.hip), where d and e are compile-time constants.  In
// scope: RT, LAG (the FL_EVAL_LAGGED scoring pass compiled in), SP (the shape policy, fl_layout.h:
// FlShapeDyn = d and e are the kernel arguments), d, e, c, b, pg, st_in, st_out, local_step,
// stage_local, mode, cm_out, fold_mask.  LAG: 0 no lagged scoring, 1 scoring pass before the
// training pass, 2 scoring in registers on the last FL_LAG_SPR RT waves beside it (score_out),
// 3 the same scoring on workgroups of its own (score_block_bf16): blocks [n_slabs, 2 n_slabs) of
// a lagged round score, blocks [0, n_slabs) train exactly as a non-lagged round (LAG 0).
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ FLState S_sh;
    __shared__ int dgrad_done;  // backward: dgrad waves finished so far (see the loop below)
    __shared__ int fwd_done;    // LAG 2: forward-phase arrivals of the training waves
    // LAG 2 / 3: per 16-row group, the logits partials of its upper scoring waves + their ready count
    __shared__ f32x4 lag_parts[(LAG == 2 || LAG == 3) ? RT * (FL_LAG_SPR - 1) * FL_LAG_PARTS * 16 : 1];
    __shared__ int lag_ready[(LAG == 2 || LAG == 3) ? RT : 1];
    if constexpr (LAG == 3) {
        if (mode == FL_EVAL_LAGGED && local_step == 0 && (int)blockIdx.x >= c.n_slabs) {
            score_block_bf16<RT>(d, e, c, b, st_in, cm_out, lds, lag_parts, lag_ready);
            return;
        }
    }
    // (what the training blocks compile: LAG 3's train like LAG 0)
    constexpr int LAGT = LAG == 3 ? 0 : LAG;
    FL_STAMP(0);
    if (threadIdx.x == 0) {  // (ordered before their first use by the staging barrier)
        dgrad_done = 0;
        if constexpr (LAGT == 2) {
            fwd_done = 0;
            for (int i = 0; i < RT; ++i) lag_ready[i] = 0;
        }
    }
    int* cm_s = reinterpret_cast<int*>(lds + e.cm_off);
    const int C = d.dim[d.L];
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
                // FUSED / FUSED_SKIP / LAGGED: the Adam kernel folds the previous round and
                // decides; train on the tentative decision (a stop only turns this round into a
                // no-op later)
                S0.live = (!S0.stopped && S0.next_round < c.max_rounds) ? 1 : 0;
            }
        }
        if (threadIdx.x == 0) {
            S_sh = S0;
            // score the rows for the previous round iff its metrics are still pending
            cm_s[FL_CM_FLAG] = (local_step == 0 && mode == FL_EVAL_FUSED && S0.next_round > S0.finalized) ? 1 : 0;
        }
    }
    for (int i = threadIdx.x; i < C * C; i += FL_THREADS) cm_s[i] = 0;
    const float* params = (local_step == 0) ? pg : b.local;
    const int R = RT * 16;
    const int row0 = blockIdx.x * R;
    const int L = d.L;
    const int ylab = (threadIdx.x < R) ? b.y[min(row0 + (int)threadIdx.x, c.n_rows - 1)] : 0;
    // FL_EVAL_LAGGED (first local step): the previous round's local model, still intact in
    // pk_local (this round's Adam has not run), is staged and scored first; the round's own
    // weights are loaded meanwhile and replace it in LDS before the training pass
    const bool lagged = LAGT && mode == FL_EVAL_LAGGED && local_step == 0;
    const char* img = (local_step == 0 && !stage_local) ? b.pk_global : b.pk_local;
    // LAG 2: the scoring waves' labels (rows row0 + 16 sw + lane % 16), loaded with the staging
    const int ysc = (LAGT == 2 && lagged && (int)(threadIdx.x >> 6) >= FL_WAVES - FL_LAG_SPR * RT)
                        ? b.y[min(row0 + 16 * (((int)(threadIdx.x >> 6) - (FL_WAVES - FL_LAG_SPR * RT)) / FL_LAG_SPR) +
                                      (int)(threadIdx.x & 15),
                                  c.n_rows - 1)]
                        : 0;
    // LAG 2, lagged rounds: the last FL_LAG_SPR RT waves score (score_in_lds + score_out) and do not stage
    constexpr int NT = LAGT == 2 ? (FL_WAVES - FL_LAG_SPR * RT) * 64 : FL_THREADS;
    const bool scorer = LAGT == 2 && lagged && (int)(threadIdx.x >> 6) >= FL_WAVES - FL_LAG_SPR * RT;
    ScoreIn sin;
    static_assert(!(LAGT == 1 && PLAIN), "the serial scoring pass stages the split image");
    ScorePre spre;
    if (LAGT == 2 && lagged) {
        if (!scorer) stage_params_rows_bf16<RT, NT, PLAIN, SP>(e, img, b.X, c.n_rows, d.dim[0], row0, lds);
        else score_prefetch<RT>(d, e, b, spre);
    } else {
        stage_params_rows_bf16<RT, FL_THREADS, PLAIN, SP>(e, (LAGT == 1 && lagged) ? b.pk_local : img, b.X, c.n_rows,
                                                      d.dim[0], row0, lds);
    }
    FL_STAMP(8);
    {   // padding columns [C, kp[L]) of D_L never change: zero them here, off the CE's path
        const int padc = e.kp[L] - C;
        uint16_t* DL = reinterpret_cast<uint16_t*>(lds + e.dlt_off[L]);
        const int nt = (LAGT == 2 && lagged) ? NT : FL_THREADS;
        if ((int)threadIdx.x < nt)
            for (int i = threadIdx.x; i < R * padc; i += nt) {
                const int r = i / padc;
                DL[r * e.lda[L] + C + (i - r * padc)] = 0;
            }
    }
    FL_STAMP(9);
    lds_barrier();
    FL_STAMP(1);
    if (!S_sh.live) return;
    float* slab = b.slab + (size_t)blockIdx.x * c.slab_stride;
    // lagged: pass 0 scores the previous local model (C:148), pass 1 trains; one call site of
    // the forward pass (inlined, so the prefetched weights stay in registers across it)
    if constexpr (LAGT == 2) {
        const int wave = threadIdx.x >> 6;
        if (!lagged) forward_block_bf16<RT, false, PLAIN, SP>(d, e, lds, b.dbg);
        else if (scorer) {
            const int sw = wave - (FL_WAVES - FL_LAG_SPR * RT);
            score_in_lds<RT>(d, e, b, lds, sw, spre, sin);
            score_out<RT>(d, e, c, b, cm_s, sw, row0, ysc, sin,
                          lag_parts + (sw / FL_LAG_SPR) * (FL_LAG_SPR - 1) * FL_LAG_PARTS * 16, lag_ready + sw / FL_LAG_SPR);
        }
        else forward_block_bf16<RT, true, PLAIN, SP>(d, e, lds, b.dbg, &fwd_done);
    } else {
    ParamRegs pr;
    if (lagged) params_load(e, img, pr);
    for (int pass = lagged ? 0 : 1; pass < 2; ++pass) {
        if (pass == 1 && lagged) {
            if (threadIdx.x < R) {
                // the scored model's argmax: counts -> b.cnt after the CE barrier below
                const int r = threadIdx.x;
                if (row0 + r < c.n_rows) {
                    const float* zr = reinterpret_cast<const float*>(lds + e.logit_off) + r * FL_LOGIT_LD;
                    int best = 0;
                    float bv = zr[0];
                    for (int k = 1; k < C; ++k)
                        if (zr[k] > bv) { bv = zr[k]; best = k; }
                    atomicAdd(&cm_s[ylab * C + best], 1);
                }
            }
            lds_barrier();  // every read of the scored image and its logits is done
            params_store(e, img, pr, lds);
            lds_barrier();
        }
        forward_block_bf16<RT, false, PLAIN, SP>(d, e, lds, b.dbg);
    }
    }
    FL_STAMP(2);

    // softmax cross-entropy: D_L = softmax - onehot, bf16, times the mean's 1/n -- except with
    // the fp16 slab, whose partials are sums of the unscaled gradient (the 1/n is applied by the
    // Adam kernel after its fp32 reduction, so small gradients keep fp16's normal range).
    // Fused evaluation: the same logits score the previous round's model (argmax).
    const float* z = reinterpret_cast<const float*>(lds + e.logit_off);
    uint16_t* DL = reinterpret_cast<uint16_t*>(lds + e.dlt_off[L]);
    const int ldL = e.lda[L];
    const bool score = cm_s[FL_CM_FLAG] != 0;
    float lossv = 0.f;
    if (threadIdx.x < R) {
        const int r = threadIdx.x, row = row0 + r;
        const float* zr = z + r * FL_LOGIT_LD;
        uint16_t* dr = DL + r * ldL;
        if (row < c.n_rows && C == 2) {
            // two classes (the reference's income label): both logits read once, the same
            // arithmetic as the general loop below in the same order (bit-identical deltas)
            const int y = ylab;
            const float z0 = zr[0], z1 = zr[1];
            const float mx = fmaxf(z0, z1);
            const int best = z1 > z0 ? 1 : 0;
            if (score) atomicAdd(&cm_s[y * 2 + best], 1);
            const float e0 = __expf(z0 - mx), e1 = __expf(z1 - mx);
            const float se = (0.f + e0) + e1;
            const float inv_se = 1.f / se;
            const float lse = mx + __logf(se);
            lossv = (lse - (y ? z1 : z0)) * c.inv_n;
            const float d0 = e0 * inv_se - (y == 0 ? 1.f : 0.f), d1 = e1 * inv_se - (y == 1 ? 1.f : 0.f);
            if constexpr (LAGT == 2) {
                *reinterpret_cast<uint32_t*>(dr) = cvt_pk_bf16(c.slab_f16 ? d0 : d0 * c.inv_n, c.slab_f16 ? d1 : d1 * c.inv_n);
            } else {
                dr[0] = (uint16_t)bf16_bits(c.slab_f16 ? d0 : d0 * c.inv_n);
                dr[1] = (uint16_t)bf16_bits(c.slab_f16 ? d1 : d1 * c.inv_n);
            }
        } else if (row < c.n_rows) {
            const int y = ylab;
            float mx = zr[0], bv = zr[0];
            int best = 0;
            for (int k = 1; k < C; ++k) {
                mx = fmaxf(mx, zr[k]);
                if (zr[k] > bv) { bv = zr[k]; best = k; }  // torch.max(dim=1): first maximum
            }
            if (score) atomicAdd(&cm_s[y * C + best], 1);
            // hardware exp2/log2 (v_exp_f32 / v_log_f32): the deltas are rounded to bf16
            // right after, far coarser than the fast intrinsics' error; the libm versions
            // were a ~1 us dependent chain per round (in-kernel stamps)
            float se = 0.f;
            for (int k = 0; k < C; ++k) se += __expf(zr[k] - mx);
            const float inv_se = 1.f / se;
            const float lse = mx + __logf(se);
            lossv = (lse - zr[y]) * c.inv_n;
            for (int k = 0; k < C; ++k) {
                const float p = __expf(zr[k] - mx) * inv_se;
                const float dk = p - (k == y ? 1.f : 0.f);
                dr[k] = (uint16_t)bf16_bits(c.slab_f16 ? dk : dk * c.inv_n);
            }
        } else {
            for (int k = 0; k < C; ++k) dr[k] = 0;
        }
    }
    if (threadIdx.x < 64) {
        lossv = wave_sum(lossv);
        if constexpr (SP::kSlabBlocked) {
            // blocked fp16 row (fl_layout.h): the loss slot follows its P halves' floats, and the row's
            // last 16-byte chunk is completed with zeros (the Adam kernel reads whole chunks)
            constexpr FlSlabBlk sb = SP::kSlabBlocked ? *SP::ps : FlSlabBlk{};  // (non-dependent SP: see FL_SHAPE_D)
            if (threadIdx.x == 0) slab[sb.P] = lossv;
            if ((int)threadIdx.x < sb.Pz - sb.P) slab_store_h(reinterpret_cast<uint16_t*>(slab) + sb.P + threadIdx.x, 0.f);
        } else {
            if (threadIdx.x == 0) slab[d.P] = lossv;
            // dense fp16 row: its last 16-byte chunk is completed with zeros as well (the Adam kernel reads
            // whole chunks and checks every half it reads for saturation); halves [P, roundup8(P)) end at or
            // before half 2 P, where the fp32 loss slot starts (P >= 4)
            if (c.slab_f16 && (int)threadIdx.x < ((-d.P) & 7))
                slab_store_h(reinterpret_cast<uint16_t*>(slab) + d.P + threadIdx.x, 0.f);
        }
    }
    lds_barrier();
    if (score || lagged)
        for (int i = threadIdx.x; i < C * C; i += FL_THREADS)
            if (cm_s[i]) atomicAdd(&cm_out[i], (float)cm_s[i]);
    FL_STAMP(3);

    // backward, top layer first, one phase per layer (wgrad_l and dgrad_l are independent).
    // A layer whose dgrad runs on waves of its own (long k-chains, wgrad_waves_bf16) ends
    // without a barrier: its dgrad waves count themselves done in LDS, and every wave starts
    // the next layer once all of them are -- the next phase reads D_l, written by the dgrad,
    // and act_{l-1}; this phase's wgrad waves still read only D_{l+1} and act_l, and the next
    // phase writes only D_{l-1} and the slab (separate buffers), so the wgrad tiles of layer l
    // overlap the next layer's work instead of holding it at a barrier.
    int dgrad_target = 0;
#pragma unroll SP::kStatic ? FL_MAX_LAYERS : 1  // static shape: one copy per layer, constants throughout
    for (int l = L - 1; l >= 0; --l) {
        const int nw = wgrad_waves_bf16<SP>(e, l);
        if (SP::kSlabBlocked || c.slab_f16) wgrad_layer_bf16<RT, true, SP>(d, e, l, lds, slab, nw);
        else wgrad_layer_bf16<RT, false, SP>(d, e, l, lds, slab, nw);
#ifdef FL_STAMP_FINE  // profiling builds only (tools/probes/stamps_fine.py): wgrad / dgrad split
        if (l == L - 2) FL_STAMP(7);
        if (l == L - 1) FL_STAMP(14);
        if (l == L - 2 && b.dbg != nullptr && threadIdx.x == 64 * (FL_WAVES - 1))  // last wave: dgrad start
            b.dbg[blockIdx.x * 16 + 11] = __builtin_amdgcn_s_memrealtime();
#endif
        if (l > 0) dgrad_layer_bf16<RT, LAGT == 2, SP>(d, e, l, lds);
#ifdef FL_STAMP_FINE
        if (l == L - 2) FL_STAMP(13);
        if (l == L - 2 && b.dbg != nullptr && threadIdx.x == 64 * (FL_WAVES - 1))  // last wave: dgrad end
            b.dbg[blockIdx.x * 16 + 12] = __builtin_amdgcn_s_memrealtime();
#endif
        if (nw < FL_WAVES && l > 0) {
            dgrad_target += FL_WAVES - nw;
            if ((int)(threadIdx.x >> 6) >= nw) lds_count_arrive(&dgrad_done);
            lds_count_wait(&dgrad_done, dgrad_target);
        } else {
            lds_barrier();
        }
        FL_STAMP(4 + (L - 1 - l));
    }
    FL_STAMP(15);
