// Body of the Adam kernel (fl_kernels.hip), included verbatim by fl_adam_kernel and
// fl_adam_batch_kernel (see fl_train_bf16_body.inc).  In scope: d, c, b, pin, anchor, comm, st,
// local_step, e, pack, st_out, fold, tail_a, fold_mask, pa, xchg, afold; macro ADAM_PA_LL: the
// exchange uses LL chunks (pa.ll != nullptr; a constant in the specialised kernels).  ADAM_BLK: the
// block's index in the Adam grid (blockIdx.x, or a virtual block of fl_adam_ll_grid_kernel).
// ADAM_STATIC / ADAM_FINALIZE / ADAM_EARLY: set by the shape-specialised kernel (fl_adam_spec.hip).
#ifndef ADAM_BLK
#define ADAM_BLK blockIdx.x
#define ADAM_BLK_DEFAULTED
#endif
#ifndef ADAM_STATIC  // the descriptors d / e are compile-time constants (fl_adam_spec.hip)
#define ADAM_STATIC false
#define ADAM_STATIC_DEFAULTED
#endif
#ifndef ADAM_FINALIZE  // the metric fold of round_state (fl_adam_spec.hip: out of line)
#define ADAM_FINALIZE(S0, hist) finalize_state(d, c, b, anchor, S0, hist, fold_mask)
#define ADAM_FINALIZE_DEFAULTED
#endif
#ifndef ADAM_EARLY  // 1: wave 0 loads the state on entry and its Adam scalars with the FedAvg weight (fl_adam_spec.hip)
#define ADAM_EARLY 0
#define ADAM_EARLY_DEFAULTED
#endif
// Slab row order.  Default: the dense row -- position p of a row is dense parameter p, d.P of them, the
// loss partial the fp32 at float index d.P.  fl_adam_spec.hip's blocked instantiation reads the blocked
// row of fl_layout.h (FlSlabBlk): ADAM_SLAB_LEN positions, ADAM_SLAB_DENSE(p) their dense index (-1: a
// pad column, its lane stays idle), ADAM_SLAB_VALID(di) whether the lane owns a parameter.  A block
// still owns 64 consecutive positions and sums them in the same order.
#ifndef ADAM_SLAB_LEN
#define ADAM_SLAB_LEN d.P
#define ADAM_SLAB_DENSE(p) (p)
#define ADAM_SLAB_VALID(di) ((di) < d.P)
#define ADAM_SLAB_DEFAULTED
#endif
#ifndef ADAM_PA_RSAG  // weight chunks by reduce-scatter + all-gather on the LL ring (peer_device.h peer_rsag)
#define ADAM_PA_RSAG false
#define ADAM_PA_RSAG_DEFAULTED
#endif
    __shared__ float part[ADAM_CANON][64];
    __shared__ FLState S_sh;
    __shared__ float lag_s[PEER_MAX_WORLD * (FL_MAX_CLASSES * FL_MAX_CLASSES + 1)];
    const int last_local_step = (local_step == c.local_steps - 1);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float sc0 = 0.f;  // parameter blocks: this step's schedule entry (rtab), read by round_state
    FL_STAMP(0);
#if ADAM_EARLY
    // The chain state -> round -> schedule entries is two dependent trips to memory on wave 0, the
    // wave that applies the update: the state load goes out first of all, and the step's Adam
    // scalars (sched) are fetched with the FedAvg weight (rtab) as soon as the round is known,
    // not after the block's barrier.
    // Wave 0 only, like its one reader round_state.  No initialiser, and the address through a
    // per-lane zero the compiler cannot see through: it moves a uniform value it has to merge or
    // knows to be uniform into scalar registers where it is loaded, and waits for the load there.
    FLState S_early;
    if (wave == 0) {
        int lane_zero;
        asm("v_mov_b32 %0, 0" : "=v"(lane_zero));
        S_early = *reinterpret_cast<const FLState*>(reinterpret_cast<const char*>(st) + lane_zero);
    }
    float sched_pre[2] = {0.f, 0.f};
#endif
    const unsigned target = st->calls + 1;  // call index of this kernel's exchanges
    // lag region A through LL slots (peer_device.h) when it fits one chunk's 64 positions:
    // every rank pushes its whole region (zeros outside its own segment), receivers sum in rank
    // order -- the same values as the pull protocol's sum
    const bool ll_lag = ADAM_PA_LL && c.tail_len <= 64;
    // Round state.  Fused evaluation (fl_common.h): wave 0 of EVERY block folds the previous
    // round's tail (anchor = this round's input image) into the previous state and decides
    // whether this round is live -- the same deterministic computation everywhere, so no
    // block waits for another; block 0 publishes it.  When the fold cannot change the decision
    // (no early stopping, or a patience counter above 2: fold_may_stop) only block 0 (history)
    // runs it.  Called after the wave issued
    // its first slab loads, so the fold's double-precision metrics overlap them.  `afold`: the
    // previous round was lagged; its metrics are region A of every rank's send buffer,
    // exchanged right here (chunk ADAM_CHUNK_LAG), so the live decision is taken in time.
    auto round_state = [&]() {
        if (wave != 0) return;
#if ADAM_EARLY
        FLState S0 = S_early;
#else
        FLState S0 = *st;
#endif
        if (ADAM_BLK != 0) {
            // the round this step belongs to whenever it is live: the folded state's next round,
            // or the running one (loaded here, after the slab loads were issued, not in front of
            // them: it depends on the state load)
            const int rg = fold ? S0.next_round : S0.cur_round;
            sc0 = b.rtab[4 * (size_t)min(max(rg, 0), c.max_rounds - 1)];
#if ADAM_EARLY
            // a live step's slot is t - 1 = cur_round * local_steps + local_step with cur_round = rg
            // (adam_update; the fold leaves next_round as it is); the clamp keeps a dead one in range
            const size_t slot = (size_t)min(max(rg, 0), c.max_rounds - 1) * c.local_steps + local_step;
            sched_pre[0] = b.sched[2 * slot];
            sched_pre[1] = b.sched[2 * slot + 1];
#endif
        }
        if (fold) {
            const bool need = ADAM_BLK == 0 || fold_may_stop(c, S0);
            if (afold) {
                if (need && ll_lag) {
                    const float lv = peer_ll_sum(pa, ADAM_CHUNK_LAG * 64 + lane, target, lane < c.tail_len);
                    if (lane < c.tail_len) lag_s[lane] = lv;
                } else if (need) {
                    peer_chunk_wait(pa, ADAM_CHUNK_LAG, target);
                    for (int i = lane; i < c.tail_len; i += 64) lag_s[i] = peer_pull_sum(pa, c.lag_off + i);
                }
                if (need) {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    S0 = fold_round(d, c, b, lag_s, S0.next_round - 1, S0, ADAM_BLK == 0);
                }
            } else if (need) {
                S0 = ADAM_FINALIZE(S0, ADAM_BLK == 0);
            }
            if (lane == 0) {
                // a stop triggered before the round that ran last (fold of region A one round
                // late): that round is discarded (fl_common.h FLState::late)
                S0.late = (!st->stopped && S0.stopped && S0.stop_round < st->next_round) ? 1 : 0;
                S0.live = (!S0.stopped && S0.next_round < c.max_rounds) ? 1 : 0;
                if (S0.live) { S0.cur_round = S0.next_round; S0.next_round += 1; }
                if (xchg || afold) S0.calls += 1;  // every rank counts its exchange calls alike
                if (ADAM_BLK == 0) *st_out = S0;
            }
        }
        if (lane == 0) S_sh = S0;
    };
    if (ADAM_BLK == 0) {
        // tail block: this rank's confusion slots are zeroed (the eval pass accumulates
        // into them); its loss slot gets the per-workgroup CE partials, summed in a fixed order
        if (!last_local_step) {
            round_state();
            return;
        }
        const int CC = c.tail_stride - 1;
        if (afold) {
            // lag region A first -- the previous round's counts (scored by this round's train
            // kernel) and loss -- published at once: every block of every rank folds from it
            for (int jj = threadIdx.x; jj < c.tail_len; jj += blockDim.x) {
                const int k = jj / c.tail_stride, e = jj - k * c.tail_stride;
                const float v = (k == c.rank) ? (e < CC ? b.cnt[e] : b.lbuf[0]) : 0.f;
                comm[c.lag_off + jj] = v;
                if (ll_lag) peer_ll_push(pa, ADAM_CHUNK_LAG * 64 + jj, target, v);  // (jj < 64: wave 0)
            }
            if (!ll_lag) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (wave == 0) peer_chunk_publish(pa, ADAM_CHUNK_LAG, target);
            }
        }
        // first batch of loss loads in flight before the fold.  Canonical order: ADAM_CANON x 64
        // virtual threads t (t = threadIdx.x + ADAM_WAVES 64 v), t summing slabs t, t + 1024, ...
        // (one per virtual thread up to 1024 slabs), the same for every block shape
        constexpr int TVW = ADAM_CANON / ADAM_WAVES;
        float lp[TVW];
#pragma unroll
        for (int v = 0; v < TVW; ++v) {
            const int s0 = threadIdx.x + ADAM_WAVES * 64 * v;
            lp[v] = s0 < c.n_slabs ? b.slab[(size_t)s0 * c.slab_stride + ADAM_SLAB_LEN] : 0.f;
        }
        round_state();
#pragma unroll
        for (int v = 0; v < TVW; ++v) {
            const int s0 = threadIdx.x + ADAM_WAVES * 64 * v;
            for (int s = s0 + ADAM_CANON * 64; s < c.n_slabs; s += ADAM_CANON * 64)
                lp[v] += b.slab[(size_t)s * c.slab_stride + ADAM_SLAB_LEN];
            part[wave + ADAM_WAVES * v][lane] = lp[v];
        }
        lds_barrier();
        const FLState S = S_sh;
        if (wave == 0) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < ADAM_CANON; ++w) t += part[w][lane];
            t = wave_sum(t);
            part[0][lane] = t;
        }
        lds_barrier();
        const float loss = part[0][0];
        for (int jj = threadIdx.x; jj < c.tail_len; jj += blockDim.x) {
            const int i = d.Pimg + jj;
            if (!S.live) {
                // past the stop: republish the input (late stop: keep the buffer's own image)
                if (c.rank != 0) comm[i] = 0.f;
                else if (!S.late) comm[i] = anchor[i];
                continue;
            }
            const int k = jj / c.tail_stride, e = jj - k * c.tail_stride;
            comm[i] = (k == c.rank && e == c.tail_stride - 1) ? loss : 0.f;
        }
        if (c.lag_off > 0) {
            // lag region A (FL_EVAL_LAGGED, FedAvg outside this kernel): the previous round's
            // counts and loss when `tail_a`, folded one round later from the all-reduce
            if (!afold)
                for (int jj = threadIdx.x; jj < c.tail_len; jj += blockDim.x) {
                    const int i = c.lag_off + jj;
                    if (!S.live) {
                        if (c.rank != 0) comm[i] = 0.f;
                        else if (!S.late) comm[i] = anchor[i];
                        continue;
                    }
                    const int k = jj / c.tail_stride, e = jj - k * c.tail_stride;
                    comm[i] = (tail_a && k == c.rank) ? (e < CC ? b.cnt[e] : b.lbuf[0]) : 0.f;
                }
            __syncthreads();  // every read of cnt / lbuf is done
            // this round's loss is kept for the next round; the counts cleared for the next
            // train kernel
            if (S.live) {
                for (int e = threadIdx.x; e < CC; e += blockDim.x) b.cnt[e] = 0.f;
                if (threadIdx.x == 0) b.lbuf[0] = loss;
            }
        }
#ifdef FL_TAIL_PULL  // (A/B builds: tails through publish / wait / pull)
        if (false) {
#else
        if (xchg && ADAM_PA_LL && c.tail_len <= 64) {
#endif
            // Adam-fused FedAvg of the metric tails on LL slots, like the weight chunks: one
            // one-way push of every tail value with the call index, a poll of this rank's own
            // ring, the sum in rank order -- instead of publish / wait / remote pull (two
            // round trips).  (The output's lag region A is not produced: after an in-kernel
            // exchange nothing folds it -- FLEngine fold masks drop FL_FOLD_A after afold.)
            // The tail values were stored by wave 0 itself (tail_len <= 64 threads).
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (wave == 0) {
                const bool act = lane < c.tail_len;
                const int pos = ADAM_CHUNK_TAIL * 64 + lane;
                if (act) peer_ll_push(pa, pos, target, comm[d.Pimg + lane]);
                const float g = peer_ll_sum(pa, pos, target, act);
                if (act) pa.out[d.Pimg + lane] = g;
            }
        } else if (xchg) {
            // Adam-fused FedAvg of the metric tails (peer_device.h)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // every wave's tail stores are acknowledged
            if (wave == 0) {
                peer_chunk_exchange_wait(pa, ADAM_CHUNK_TAIL, target);
                for (int i = d.Pimg + lane; i < (int)pa.n; i += 64) pa.out[i] = peer_pull_sum(pa, i);
            }
        }
        return;
    }
    const int pblk = ADAM_BLK - 1;
    const int di = ADAM_SLAB_DENSE(pblk * 64 + lane);  // dense index of the lane's slab position
    const bool valid = ADAM_SLAB_VALID(di);
    // dense index -> image index (and, in bf16 mode, -> packed bf16 LDS-layout position), on
    // wave 0 (the update runs there): fl_adam_map.h, shared with the host
    int j = 0, pk = 0;
    bool is_bias = false;
    if (wave == 0 && valid) {
        const FlAdamPos ps = fl_adam_pos<ADAM_STATIC>(d, e, di);
        j = ps.j;
        pk = ps.pk;
        is_bias = ps.is_bias;
    }
    // past the stop: rank 0 contributes the (identical) global weights, others 0, so the
    // all-reduce returns them bit-exactly.  Classic rounds know the state on entry and skip
    // the reduction; fused rounds learn it at the barrier below.
    if (!fold && !st->live) {
        if (wave == 0 && valid && last_local_step && !(c.rank == 0 && st->late))
            comm[j] = (c.rank == 0) ? anchor[j] : 0.f;
        return;
    }
    // wave 0's operands of the update, issued before the slab loads so their latency overlaps
    // (the schedule entry sc0 follows in round_state)
    float p0 = 0.f, m0 = 0.f, v0 = 0.f, a0 = 0.f;
    if (wave == 0 && valid) {
        p0 = pin[j];
        m0 = b.m[j];
        v0 = b.v[j];
        a0 = anchor[j];
    }
    bool have_state = false;
    // Slab reduction with 16-byte loads: lane (q, r) = (lane % LPR, lane / LPR) reads VEC
    // consecutive partials (parameters 8q..8q+7 of the block for the fp16 slab, 4q..4q+3 for
    // fp32) of slab row VEC cw + r, then rows 16 VEC further: one load instruction per row-group
    // instead of one 2-byte load per row and parameter (8x fewer, each a whole 1 KB per wave).
    // The summation order is CANONICAL -- ADAM_CANON = 16 waves cw, each summing its rows in row
    // order, an xor tree over the r bits, then the 16 waves' sums in cw order (adam_update) -- and
    // a block of ADAM_WAVES < 16 waves runs VW = 16 / ADAM_WAVES of those canonical waves per wave
    // (cw = wave + ADAM_WAVES v), so every block shape gives bit-identical gradients (the trial
    // batches' 4-wave blocks = the single engine's 16-wave blocks).  Groups past the block's last
    // parameter read row offset 0.
// Slab rows: default-policy loads.  Nontemporal loads (FL_ADAM_NT_LOADS, rounds 1-4) cost
// 0.2 us per one-client round and 1.2 us per emulated N > 1 round at 8000 rows
// (profiles/adam_slab_load_policy_r5.log); the train kernel's fp16 slab stores are write-through
// (fl_device.h slab_store_h; default-policy stores: +1.3 us).
#if defined(FL_ADAM_NT_LOADS)
#define FL_SLAB_LD(p) __builtin_nontemporal_load(p)
#elif defined(FL_SLAB_AUX)
// (A/B builds: slab rows through buffer loads with cache-policy bits FL_SLAB_AUX, e.g. 17 = sc0 sc1)
#define FL_SLAB_LD(p) fl_slab_ld_aux(b.slab, p)
#else
#define FL_SLAB_LD(p) (*(p))
#endif
// FL_PROBE_SLAB_ROWS=k (timing probes only, profiles/adam_slab_floor_r6.log): read only the first
// k slab rows -- bounds the Adam kernel's time without (part of) its slab read.  Wrong values.
#ifdef FL_PROBE_SLAB_ROWS
#define FL_NSL min(c.n_slabs, FL_PROBE_SLAB_ROWS)
#else
#define FL_NSL c.n_slabs
#endif
#define FL_SLAB_REDUCE_WIDE(VT, ET, VEC)                                                            \
    {                                                                                               \
        constexpr int LPR = 64 / (VEC), VW = ADAM_CANON / ADAM_WAVES;                               \
        const int q = lane & (LPR - 1), r = lane / LPR;                                             \
        const int p0i = pblk * 64 + q * (VEC);                                                      \
        const ET* base = reinterpret_cast<const ET*>(b.slab) + (p0i < ADAM_SLAB_LEN ? p0i : 0);     \
        const size_t rs = (size_t)c.slab_stride * (sizeof(float) / sizeof(ET)); /* ET per row */    \
        float acc[VW][VEC];                                                                         \
        bool sat = false; /* fp16 slab: a saturated (clamped) or non-finite partial was read */     \
        _Pragma("unroll") for (int v = 0; v < VW; ++v)                                              \
            _Pragma("unroll") for (int i = 0; i < (VEC); ++i) acc[v][i] = 0.f;                      \
        for (int k0 = 0; k0 * ADAM_CANON * (VEC) < FL_NSL; k0 += ADAM_WDEPTH) {                  \
            VT x[VW][ADAM_WDEPTH];                                                                  \
            _Pragma("unroll") for (int v = 0; v < VW; ++v)                                          \
                _Pragma("unroll") for (int u = 0; u < ADAM_WDEPTH; ++u) {                           \
                    const int sr = (VEC) * (wave + ADAM_WAVES * v) + r + ADAM_CANON * (VEC) * (k0 + u); \
                    const VT ld = FL_SLAB_LD(                                                       \
                        reinterpret_cast<const VT*>(base + (size_t)(sr < FL_NSL ? sr : 0) * rs)); \
                    _Pragma("unroll") for (int i = 0; i < (VEC); ++i)                               \
                        x[v][u][i] = sr < FL_NSL ? ld[i] : (ET)0;                                   \
                }                                                                                   \
            if (!have_state) {                                                                      \
                have_state = true;                                                                  \
                FL_STAMP(1);                                                                        \
                round_state();                                                                      \
                FL_STAMP(2);                                                                        \
            }                                                                                       \
            _Pragma("unroll") for (int v = 0; v < VW; ++v)                                          \
                _Pragma("unroll") for (int u = 0; u < ADAM_WDEPTH; ++u)                             \
                    _Pragma("unroll") for (int i = 0; i < (VEC); ++i) {                             \
                        const float xf = (float)x[v][u][i];                                         \
                        if (sizeof(ET) == 2) sat |= !(fabsf(xf) < 65504.f);                         \
                        acc[v][i] += xf;                                                            \
                    }                                                                               \
        }                                                                                           \
        if (sizeof(ET) == 2 && sat && b.sat != nullptr) *b.sat = 1; /* benign race: all write 1 */  \
        _Pragma("unroll") for (int v = 0; v < VW; ++v)                                              \
            _Pragma("unroll") for (int off = LPR; off < 64; off <<= 1)                              \
                _Pragma("unroll") for (int i = 0; i < (VEC); ++i) acc[v][i] += __shfl_xor(acc[v][i], off, 64); \
        if (r == 0)                                                                                 \
            _Pragma("unroll") for (int v = 0; v < VW; ++v)                                          \
                _Pragma("unroll") for (int i = 0; i < (VEC); ++i)                                   \
                    part[wave + ADAM_WAVES * v][q * (VEC) + i] = acc[v][i];                         \
    }
    if (c.slab_f16) {
        FL_SLAB_REDUCE_WIDE(fl_half8, _Float16, 8)
    } else {
        FL_SLAB_REDUCE_WIDE(fl_float4v, float, 4)
    }
#undef FL_SLAB_REDUCE_WIDE
#undef FL_NSL
#undef FL_SLAB_LD
    if (!have_state) round_state();
    FL_STAMP(3);
    lds_barrier();
    if (wave != 0) return;
    FL_STAMP(4);
    const FLState S = S_sh;
    float contrib = 0.f;  // this rank's FedAvg contribution of the lane's parameter
    if (valid) {
        if (!S.live) {
            // (a late stop never happens with the in-kernel exchange: it folds in time)
            contrib = (c.rank == 0) ? (S.late ? comm[j] : a0) : 0.f;
            if (last_local_step && !(c.rank == 0 && S.late)) comm[j] = contrib;
            if (S.late && b.undo != nullptr) undo_restore(c, b, pack, j, pk, is_bias, e.wlo_delta);
        } else {
#if ADAM_EARLY
            contrib = adam_update(c, b, comm, S, local_step, last_local_step, pack, j, pk, is_bias, e.wlo_delta, part,
                                  lane, p0, m0, v0, a0, sc0, sched_pre);
#else
            contrib = adam_update(c, b, comm, S, local_step, last_local_step, pack, j, pk, is_bias, e.wlo_delta, part,
                                  lane, p0, m0, v0, a0, sc0);
#endif
        }
    }
    FL_STAMP(5);
    if (xchg && ADAM_PA_LL) {
        // Adam-fused FedAvg of this block's 64 parameters, LL chunks (peer_device.h): push the
        // contribution with the call index into every rank's ring, poll this rank's ring, sum
        // in rank order; global image + packed bf16 image
        const int pos = (ADAM_CHUNK_W0 + pblk) * 64 + lane;
        float gsum;
        if (ADAM_PA_RSAG) {
            gsum = peer_rsag(pa, ADAM_CHUNK_W0 + pblk, pos, target, valid, contrib);
        } else {
            if (valid) peer_ll_push(pa, pos, target, contrib);
            gsum = peer_ll_sum(pa, pos, target, valid);
        }
        if (valid) {
            pa.out[j] = gsum;
            if (pack) pack_store(b.pk_global, pk, is_bias, e.wlo_delta, gsum);
        }
    } else if (xchg) {
        // Adam-fused FedAvg of this block's 64 parameters (peer_device.h): publish, wait for
        // every rank's chunk, pull + sum in rank order; global image + packed bf16 image
        peer_chunk_exchange_wait(pa, ADAM_CHUNK_W0 + pblk, target);
        if (valid) {
            const float gsum = peer_pull_sum(pa, j);
            pa.out[j] = gsum;
            if (pack) pack_store(b.pk_global, pk, is_bias, e.wlo_delta, gsum);
        }
    }
    if (b.dbg != nullptr) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // stamp the stores' completion
    FL_STAMP(15);
#ifdef ADAM_BLK_DEFAULTED
#undef ADAM_BLK
#undef ADAM_BLK_DEFAULTED
#endif
#ifdef ADAM_SLAB_DEFAULTED
#undef ADAM_SLAB_LEN
#undef ADAM_SLAB_DENSE
#undef ADAM_SLAB_VALID
#undef ADAM_SLAB_DEFAULTED
#endif
#ifdef ADAM_PA_RSAG_DEFAULTED
#undef ADAM_PA_RSAG
#undef ADAM_PA_RSAG_DEFAULTED
#endif
#ifdef ADAM_EARLY_DEFAULTED
#undef ADAM_EARLY
#undef ADAM_EARLY_DEFAULTED
#endif
#ifdef ADAM_STATIC_DEFAULTED
#undef ADAM_STATIC
#undef ADAM_STATIC_DEFAULTED
#endif
#ifdef ADAM_FINALIZE_DEFAULTED
#undef ADAM_FINALIZE
#undef ADAM_FINALIZE_DEFAULTED
#endif
