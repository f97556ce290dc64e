// Shared host/device declarations of the fused federated-round engine.
//
// One client per GPU keeps everything resident: the local shard, the parameters, the Adam
// moments (which persist across rounds), a per-block gradient slab, and a small
// device-side round state that carries the early-stopping rule
// (FL_CustomMLPCLassifierImplementation_Multiple_Rounds.py:181-192) so the host never has to
// read metrics back to decide whether to continue.
//
// Parameter "image" layout.  Every parameter-shaped device buffer (global/comm, local, m, v)
// stores, per layer l, W_l ([N][K], torch Linear layout) as fl_wrows(N) rows of fl_ldw(K)
// floats followed by b_l padded to roundup16(N), all padding zero; W_l[n][k] sits at column
// k ^ fl_swz(n) of row n (the fp32 kernels' LDS chunk swizzle, fl_kernels.hip).  The image is
// exactly the LDS image the fp32 kernels compute from, so staging a model into LDS is one
// contiguous float4 copy, and every MFMA operand read of a 16x16 tile / 16-deep k chunk is in
// bounds and reads zeros in the padding (no predication, no exec-mask branches in inner loops).  The dense
// reference layout (named_parameters() order: model.0.weight, model.0.bias, ...; C:93-99)
// exists only at the API boundary (get/set weights, checkpoints) and in the gradient slab.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_round_plan.h"  // host-only: launch vocabulary shared with the round planner

#define FL_MAX_LAYERS 4
#define FL_MAX_CLASSES 16
#define FL_MAX_WORLD 64
// Dynamic LDS a fused-kernel workgroup may request: the CU's 160 KiB minus room for the
// kernels' small static __shared__ objects (round state, counters).
#define FL_LDS_DYNAMIC_MAX (160 * 1024 - 2048)
// Threads of a fused-kernel workgroup (overridable for variant builds: -DFL_THREADS=...).
#ifndef FL_THREADS
#define FL_THREADS 1024
#endif
#define FL_WAVES (FL_THREADS / 64)
// Lagged rounds scored in registers (fl_layout.h fl_lag_reg_ok): FL_LAG_SPR waves per 16-row
// group split the last hidden layer; each upper one hands at most FL_LAG_PARTS logits partials
// (C <= 4 classes) to the group's first wave through LDS.
#ifndef FL_LAG_SPR
#define FL_LAG_SPR 3
#endif
#define FL_LAG_PARTS (FL_LAG_SPR == 2 ? 4 : 2)
#define FL_LAG_MAX_C 4
// logits part range of scoring wave j of a group (parts [fl_lag_w(G, j), fl_lag_w(G, j + 1)))
__host__ __device__ constexpr int fl_lag_w(int G, int j) { return G - ((FL_LAG_SPR - j) * G) / FL_LAG_SPR; }

// ldw = roundup16(K) + 4 (4 mod 8 floats): 16-byte aligned rows; with the chunk swizzle
// (fl_swz below) the rows of every gfx950 ds_read_b128 lane group land on distinct 16-byte
// bank slots.
__host__ __device__ constexpr int fl_ldw(int K) { return ((K + 15) & ~15) + 4; }
__host__ __device__ constexpr int fl_wrows(int N) { return (N + 15) & ~15; }
// fp32 LDS / image chunk swizzle: row r keeps logical column k < roundup16(width) at column
// k ^ fl_swz(r) -- the 4-float chunks of rows 4..11 (mod 16) trade places in pairs
// (fl_kernels.hip; models/mlp.py mirrors it).
__host__ __device__ constexpr int fl_swz(int r) { return ((r + 4) & 8) >> 1; }

struct MLPDesc {
    int L;                            // number of Linear layers
    int dim[FL_MAX_LAYERS + 1];       // dim[0] = features, dim[L] = classes
    int ld[FL_MAX_LAYERS + 1];        // LDS leading dimension (floats) per activation buffer
    int act_off[FL_MAX_LAYERS + 1];   // LDS float offset of each activation buffer (R rows)
    int dlt_off[FL_MAX_LAYERS + 1];   // LDS float offset of the backward delta of hidden layer l
    int w_off[FL_MAX_LAYERS];         // dense (reference) offset of W_l
    int b_off[FL_MAX_LAYERS];         // dense offset of b_l
    int P;                            // dense parameter count
    int iw_off[FL_MAX_LAYERS];        // image offset of W_l
    int ib_off[FL_MAX_LAYERS];        // image offset of b_l
    int Pimg;                         // image floats (multiple of 4)
    int img_lds;                      // LDS float offset of the staged image
    int cm_off;                       // LDS float offset of the C x C int confusion counters
    int lds_floats;                   // LDS floats needed per block
};

// (dense index <-> image position, fl_image_index / fl_image_lim: fl_image.h)

// bf16 LDS layout of the fused kernels (fl_kernels_bf16.hip).  All offsets are BYTES into
// the dynamic LDS window.  Every fan-in dimension is padded to kp = roundup32(dim) (one
// v_mfma_f32_16x16x32_bf16 k-step per 32).  W_l has kp[l+1] rows (the dgrad contraction
// runs over its padded fan-out), activations / deltas have R rows.  Transposed operands (wgrad
// over rows, dgrad over W's rows) are read with ds_read_b64_tr_b16 from the same images.
//
// Bank conflicts (64 banks x 4 B; ds_read_b128 serves 16 lanes per LDS cycle,
// ds_read_b64_tr_b16 32 lanes; tests/native/test_layout.cpp models both).  Three layout
// levels, the best that fits the CU's LDS (fl_layout.h):
//   * activation / delta rows lda = kp + 16 elements (levels 1, 2): a row stride of an odd
//     multiple of 32 bytes, on which a b128 group (16 rows x 16 B) and a transposed read of 8
//     CONSECUTIVE rows x 32 B both tile the 256-byte bank period exactly.  wgrad takes its 32
//     row-k's as runs 4g..4g+3 / 16+4g..16+4g+3 per 16-lane group g (same order in both
//     operands), so each transposed read covers 8 consecutive rows.  Level 0: kp + 8.
//   * W images: row n at fl_wrow(n) = n*ldw*2 + (n/8)*wgap bytes, its 16-byte chunk c stored
//     at chunk c ^ (wxor * bit 3 of n); lane lr of a forward tile reads W row
//     fl_fwd_col(lr) = (lr + 4) & 15 and produces that output column.  Level 2: ldw = kp + 16,
//     wgap 128, wxor 0 -- dgrad's transposed reads of rows {0-3, 8-11} (k-runs tied to the b128
//     rows of the delta operand) land half a bank period apart, every read is conflict free.
//     Levels 0/1: ldw = kp + 8, no gap, wxor 1 -- the forward reads are conflict free, dgrad's
//     transposed W reads 2-way (the 10 KB of gaps and pads do not fit beside R = 32 rows of a
//     (50, 200) model).
//
// Split-bf16 forward ("bf16x3").  Every forward pass computes z = a.W^T as
// a_hi.W_hi^T + (a_lo.W_hi^T + a_hi.W_lo^T) with x_hi = bf16(x), x_lo = bf16(x - x_hi), fp32
// accumulation: ~16 significant bits per product instead of 8.  The backward pass stays plain
// bf16 (hi parts).  Reason: the reference's early-stop rule (C:181-192, atol 1e-4 on 8000-row
// accuracies) needs 10 rounds without a single prediction flip; with 8-bit scoring every
// bf16 rounding step of a changing weight flips borderline rows and the rule never fires
// (tools/bf16_es_emulate.py: split-bf16 forward stops at rounds 175-238, the fp32 oracle at
// 157-227, the reference at 149-243).  The lo images of the weights sit in the parameter
// region `wlo_delta` bytes after their hi images (same layout); the lo parts of the layer
// inputs live in `alo_off` buffers (X lo: its own buffer; hidden layers: the backward delta
// buffers, unused during the forward pass).
struct MLPDescB {
    int kp[FL_MAX_LAYERS + 1];        // roundup32(dim[l])
    int lda[FL_MAX_LAYERS + 1];       // row stride (elements) of act_l, D_l: kp[l] + 16 (level 0: + 8)
    int ldw[FL_MAX_LAYERS];           // row stride (elements) of W_l: kp[l] + 16 (level 2) or + 8
    int wgap;                         // bytes after every 8 W rows (level 2: 128)
    int wxor;                         // W chunk swizzle (levels 0/1: 1)
    int level;                        // bank layout level (2 = conflict free, see above)
    int w_off[FL_MAX_LAYERS];         // W_l  bf16 kp[l+1] rows, fl_wbyte() positions (hi parts)
    int bias_off[FL_MAX_LAYERS];      // b_l  fp32 [kp[l+1]] (zero padded)
    int wlo_delta;                    // W_l lo parts at w_off[l] + wlo_delta (same layout)
    int act_off[FL_MAX_LAYERS + 1];   // act_l bf16 [R][lda[l]]   (l < L), hi parts
    int alo_off[FL_MAX_LAYERS + 1];   // act_l lo parts bf16 [R][lda[l]] (l < L; forward pass only)
    int dlt_off[FL_MAX_LAYERS + 1];   // D_l  bf16 [R][lda[l]]    (1 <= l <= L): dLoss/dz_l
    int logit_off;                    // fp32 [R][FL_LOGIT_LD] classifier logits (16 columns)
    int head_split;                   // logits layer: K split over this many waves (1 = one wave)
    int part_off;                     // ... their fp32 partial logits [head_split][R][C]
    int cm_off;                       // int [16][16] confusion counters (fused evaluation)
    int item_base[FL_MAX_LAYERS + 1]; // packing: prefix sums of the 8-element items of each W_l
    int param_off;                    // start of the parameter region (all W_l hi, all b_l, all W_l lo):
    int param_bytes;                  // it is stored pre-packed in global memory and staged by a copy
    int lds_bytes;
    int lag_reg;                      // 1: lagged rounds score in registers (fl_layout.h fl_lag_reg_ok)
};

// Packed bf16 W images (see the bank notes above): byte offset of row n (fl_wrow(kp rows) =
// image bytes), the chunk swizzle of row n, the byte position of element (n, k), and the W
// row / output column that lane lr of a forward tile computes.
__host__ __device__ constexpr int fl_wrow(int n, int ldw, int wgap) { return n * ldw * 2 + (n >> 3) * wgap; }
__host__ __device__ constexpr int fl_wswz(int n, int wxor) { return ((n >> 3) & 1) * wxor; }
__host__ __device__ inline int fl_wbyte(const MLPDescB& e, int l, int n, int k) {
    return fl_wrow(n, e.ldw[l], e.wgap) + ((((k >> 3) ^ fl_wswz(n, e.wxor)) << 4) | ((k & 7) << 1));
}
__host__ __device__ inline int fl_fwd_col(int lr) { return (lr + 4) & 15; }
// The 4 accumulator rows of an MFMA lane (4g + j, 16-lane group g) go to LDS in 4 writes; in
// write t a lane of an odd group writes row 4g + ((t + 1) & 3), so the two 16-lane groups of a
// 32-lane write half are 5 or 1 rows apart instead of 4 (4 rows = 0 mod the 128-byte write
// bank period at these strides).
__host__ __device__ inline int fl_out_row(int lg, int t) { return 4 * lg + ((t + (lg & 1)) & 3); }
// Logit rows: 17 floats apart (one row per lane in the loss epilogue: distinct banks).
#define FL_LOGIT_LD 17

struct FLConfig {
    int R;              // rows per workgroup (16 or 32)
    int n_rows;         // local training rows
    float inv_n;        // 1 / n_rows  (CrossEntropyLoss 'mean', C:43)
    int world;
    int rank;
    float agg_scale;    // n_rank / N_total (sample-size-weighted FedAvg, C:110-116)
    int slab_stride;    // floats per slab row (dense P + loss slot, padded; an engine with blocked fp16
                        // rows: the blocked row's P, fl_layout.h FlSlabBlk)
    int n_slabs;        // workgroups of the train kernel = ceil(n_rows / R)
    int slab_f16;       // bf16 kernels: the slab holds fp16 partial SUMS (the 1/n is applied by
                        // Adam after the fp32 reduction; fl_device.h slab_store_h)
    int tail_off;       // == Pimg: start of the per-rank metric tail in the comm buffer
    int tail_stride;    // C*C confusion counts + 1 loss slot
    int tail_len;       // world * tail_stride
    int lag_off;        // > 0: start of the lag region A (tail_len floats, FL_EVAL_LAGGED)
    int plain_fwd;      // bf16, several clients, register scoring: the TRAINING forward pass is plain
                        // bf16 (a_hi.W_hi) and stages only the hi images -- every scoring pass is a
                        // separate split-bf16 forward there (fl_kernels_bf16.hip)
    int split_score;    // lagged rounds score on n_slabs workgroups of their own (train kernel LAG 3)
                        // instead of on waves of the training workgroups (LAG 2): small shards
    int local_steps;    // optimizer steps per round (reference: 1 full-batch step, C:63-73)
    // optimizer (torch.optim.Adam + StepLR, C:44-46); scalars kept in double like torch
    double lr0;
    double gamma;
    int step_size;
    double beta1;
    double beta2;
    float omb1;         // (float)(1 - beta1)  lerp weight
    float omb2;         // (float)(1 - beta2)  addcmul value
    float beta2f;       // (float)beta2
    float eps;
    float weight_decay; // L2 on the gradient (torch Adam weight_decay / sklearn alpha)
    float prox_mu;      // FedProx proximal coefficient (0 = FedAvg)
    // early stopping (C:122, C:181-192)
    int es_enabled;
    int patience;
    double atol;
    double rtol;
    int max_rounds;
    int metric_mode;    // 0 = mean of per-client metrics (C:169), 1 = pooled confusion (S:130)
};

// Device-resident round state; double-buffered by round parity so every workgroup of the
// train kernel can recompute the stop decision from an immutable input copy.
struct FLState {
    int next_round;     // index of the next round to run
    int finalized;      // rounds whose metrics have been folded into the history
    int stopped;        // early-stop signal (C:132-136 / C:189)
    int live;           // this launch's round is live (not past the stop)
    int cur_round;      // index of the round running now (valid when live)
    int count;          // patience counter (termination_count, C:125)
    int has_prev;
    int stop_round;     // round index at which the stop took effect (-1 = none)
    unsigned calls;     // Adam-fused FedAvg exchanges done (call index of the chunk flags, peer_device.h)
    // 1: this round's fold found a stop triggered by round next_round - 2 (lag region A folded one
    // round late: lagged rounds over an external all-reduce with early stopping), so round
    // next_round - 1 ran past the stop.  Its output is discarded: the round republishes the image
    // still held by its own comm buffer -- round next_round - 2's all-reduced output (the comm
    // buffer of round q is the output buffer of round q - 2) -- instead of its input.
    int late;
    double prev[4];     // prev_metric (C:126)
};

struct FLBuffers {
    const float* X;     // [n_rows, dim0] row-major, device resident
    const int* y;       // [n_rows]
    float* slab;        // [n_slabs, slab_stride] dense gradient partials (fp32; slab_f16: fp16 in the
                        // first P halves of each row, zeros up to the next multiple of 8 halves -- the Adam
                        // kernel reads 16-byte chunks --, the loss partial stays the fp32 at [P]; the
                        // reference shape's specialised train / Adam pair keeps the fp16 row blocked
                        // instead, fl_layout.h FlSlabBlk)
    float* local;       // [Pimg] post-step local weights (evaluated, C:148)
    float* m;           // [Pimg] Adam exp_avg
    float* v;           // [Pimg] Adam exp_avg_sq
    double* hist_global;  // [max_rounds, 4]
    double* hist_rank;    // [max_rounds, world, 4]
    float* hist_loss;     // [max_rounds] mean CE over clients
    unsigned long long* dbg;  // optional [blocks, 16] s_memrealtime phase stamps (profiling)
    char* pk_global;    // bf16 mode: packed LDS-layout image of the round's input weights
    char* pk_local;     // bf16 mode: packed LDS-layout image of the local (post-Adam) weights
    // Adam + StepLR scalars per optimizer step slot t = 1 .. max_rounds * local_steps (slot of
    // round r, local step ls: r * local_steps + ls + 1), computed on the host in double exactly
    // as torch does (python float pow): [t-1] = {step_size, sqrt(bias_correction2)} rounded to
    // fp32, with the bias corrections of the CLIENT'S OWN Adam step count (= t without client
    // sampling) and the LR of the round.  A table lookup instead of three double pow() on the
    // Adam kernel's critical path.
    const float* sched;
    // Per-round FedAvg table [max_rounds][4] = {this client's aggregation weight (n_i / sum of
    // the round's sampled n_j; 0 when not sampled), sampled-client count, sampled-rank bitmask
    // bits 0-31, bits 32-63 (bit patterns stored in the float slots)}.  Full participation:
    // {n_i / N, world, all ones}.  Built on the host from the seeded per-round client sample
    // (fedmi/fl/engine.py participants()), identical on every rank.
    const float* rtab;
    float* cnt;         // FL_EVAL_LAGGED: confusion counts of the previous round's local model
    float* lbuf;        // FL_EVAL_LAGGED: the previous round's loss, published one round later
    // Late fold (FLState::late; lagged rounds over an external all-reduce with early stopping):
    // [local | m | v] (3 x Pimg floats) and the packed local image (undo_pk_bytes) as they were
    // before the last live round's first optimizer step, written by adam_update; a round found
    // to have run past the stop restores them, so the local model and the Adam moments match a
    // run that stopped in time.  nullptr: no round can be discarded.
    float* undo;
    int undo_pk_bytes;
    int* sat;           // optional: set to 1 by the Adam kernel when an fp16 slab partial it reads is
                        // saturated (|x| = 65504, slab_store_h's clamp) or not finite
};

// (evaluation placement FL_EVAL_*, fold regions FL_FOLD_*: fl_round_plan.h)
// LDS confusion-counter region of the train kernels: C*C counters + a "score rows" flag,
// padded to a multiple of 16 bytes.
#define FL_CM_FLAG (FL_MAX_CLASSES * FL_MAX_CLASSES)
#define FL_CM_INTS (FL_CM_FLAG + 4)

// Trial batches (BASELINE config 5, fedmi/hpo/fed_sweep.py): K engines of the same shape --
// same layer sizes, R, rows (one client's shard), dtype -- that differ in hyperparameters (lr,
// local steps, FedProx mu, ...) advance in lock-step, and every kernel of a round runs ONCE for
// all of them with a trial grid dimension (blockIdx.y = trial) instead of K launches.  Each
// trial's configuration, buffers and the pointer bases its launches refer to sit in a device
// table; a launch names each pointer argument as (base slot, byte offset), the same for every
// trial of the batch (the recording engine checks that, fl_engine.cpp TrialBatch).
// (slots FL_TB_* and the selector FLSel: fl_round_plan.h)
struct FLTrialDesc {
    FLConfig c;
    FLBuffers b;
    char* base[FL_TB_BASES];
};
__host__ __device__ inline char* fl_sel(const FLTrialDesc& t, FLSel s) {
    return s.base < 0 ? nullptr : t.base[s.base] + s.off;
}

// Differential privacy (fl_dp.hip): parameters of the per-round clip + noise kernel, passed to
// that kernel alone (FLConfig / FLBuffers are by-value arguments of every round kernel).
struct FLDp {
    float clip;          // L2 bound S of a client's round update (> 0)
    int noise;           // 1: Gaussian noise of std sigma[round] on every real parameter
    int rank;            // third word of the noise counter
    int max_rounds;      // entries of sigma / norm_hist
    uint32_t key0, key1; // Philox key: the engine's 64-bit seed, low and high word
    const float* sigma;  // [max_rounds] z * S * max_j w_j(r) / sqrt(K_r), host-built
    float* norm_hist;    // [max_rounds] pre-clip ||local - input||_2 of this client (0: not sampled)
};

// Server optimizer (fl_server.hip): parameters of the per-round server step, passed to that
// kernel alone, as FLDp is.  With x the image the round trained from, a the aggregated image and
// d = a - x, the kernel keeps m (and, adaptive kinds, v) across rounds and replaces a by
//   FL_SERVER_SGD     : m = b1 m + d;            x + lr m                      (FedAvgM)
//   FL_SERVER_ADAGRAD : m = b1 m + (1 - b1) d;   v = v + d^2;                  x + lr m / (sqrt(v) + tau)
//   FL_SERVER_ADAM    : same m;                  v = b2 v + (1 - b2) d^2;      same step
//   FL_SERVER_YOGI    : same m;                  v = v - (1 - b2) d^2 sign(v - d^2); same step
// (Reddi et al. 2021, Algorithm 2: no bias correction, v starts at tau^2).
#define FL_SERVER_NONE 0
#define FL_SERVER_SGD 1
#define FL_SERVER_ADAGRAD 2
#define FL_SERVER_ADAM 3
#define FL_SERVER_YOGI 4
struct FLServer {
    int kind;            // FL_SERVER_*
    int max_rounds;      // rounds past it are not stepped
    float lr;            // server learning rate
    float b1;            // momentum
    float omb1;          // (float)(1 - b1)
    float b2;            // second-moment decay (Adam, Yogi)
    float omb2;          // (float)(1 - b2)
    float tau;           // adaptivity (added to sqrt(v)); v starts at tau^2
    float* m;            // [Pimg] fp32, caller-owned
    float* v;            // [Pimg] fp32, caller-owned (adaptive kinds; unused by FL_SERVER_SGD)
};

// Update compression with error feedback (fl_compress.hip): parameters of the per-round compression
// kernel, passed to that kernel alone, as FLDp is.  With x the image the round trained from and e the
// residual, u = (local - x) + e on the P real parameters and the contribution becomes w (x + C(u)):
//   FL_COMPRESS_TOPK : C keeps the k entries of largest |u| (ties: lower dense index first), e' = u elsewhere
//   FL_COMPRESS_SIGN : C(u) = copysign(s, u), s = sum|u| / P;                              e' = u - C(u)
// (Stich et al. 2018; Karimireddy et al. 2019).  The exchange still carries the dense image.
// The two stochastic kinds draw, for dense parameter p, word p % 4 of Philox4x32-10 at counter
// (p / 4, round, client, FL_QSGD_STREAM / FL_RANDK_STREAM) under (key0, key1); the round comes from the
// device state, so a replayed graph draws fresh words:
//   FL_COMPRESS_QSGD  : norm = sqrt(sum u^2); level = floor(a) + ((word >> 8) < frac(a) 2^24), a = min(|u| / norm * levels,
//                       levels); C(u) = copysign(norm * level / levels, u), e' = u - C(u); norm 0 or not finite: C(u) = u
//   FL_COMPRESS_RANDK : C keeps the k entries of largest word >> 1 (ties: lower dense index first); with error
//                       feedback C(u) = u there and e' = u elsewhere, without it C(u) = u * (P / k) there (unbiased)
// (Alistarh et al. 2017; Stich et al. 2018).
#define FL_COMPRESS_NONE 0
#define FL_COMPRESS_TOPK 1
#define FL_COMPRESS_SIGN 2
#define FL_COMPRESS_QSGD 3
#define FL_COMPRESS_RANDK 4
#define FL_COMPRESS_MAX_LEVELS 32767
#define FL_QSGD_STREAM 0x44475351u   // distinct from each other, the DP noise stream 0x46454450 (fl_dp.hip)
#define FL_RANDK_STREAM 0x4B444E52u  // and FL_SECAGG_STREAM
struct FLCompress {
    int kind;            // FL_COMPRESS_*
    int k;               // top-k: entries kept, 1 .. P
    int P;               // dense parameter count (== MLPDesc::P)
    int error_feedback;  // 1: what C drops is carried in the residual; 0: the residual stays 0
    int max_rounds;      // entries of stat_hist; rounds past it are not live
    float* residual;     // [2][Pimg] fp32, caller-owned, zero at start: round r reads half r & 1 and writes
                         // half (r + 1) & 1 (every workgroup reads the whole old residual, fl_compress.hip)
    float* stat_hist;    // [max_rounds] top-k: magnitude of the k-th kept entry; sign: s; qsgd: the norm; randk:
                         // (word >> 1) 2^-31 of the k-th kept entry (0: not sampled)
    int levels;          // qsgd: quantisation levels s, 1 .. FL_COMPRESS_MAX_LEVELS
    int client;          // stochastic kinds: third word of the counter (the rank / client index, as FLDp::rank)
    uint32_t key0, key1; // stochastic kinds: Philox key, the client's 64-bit compress seed, low and high word
};

// Robust aggregation (fl_robust.hip; Yin et al. 2018): parameters of the per-round coordinate-wise
// median / trimmed mean over K clients' buffers, passed to that kernel alone.  Of the round's K_r
// sampled clients (rtab mask) the fl_robust_trim lowest and highest values of every coordinate are
// dropped, the rest averaged.
#define FL_ROBUST_MEDIAN 1
#define FL_ROBUST_TRIMMED 2
#define FL_ROBUST_MAX_K 64           // width of the rtab mask
struct FLRobust {
    int kind;            // FL_ROBUST_*
    int K;               // sources, 1 .. FL_ROBUST_MAX_K
    int max_rounds;      // rounds of rtab; rounds past it are not live
    double beta;         // trimmed mean: fraction cut at each end, in [0, 0.5)
    const float* rtab;   // a client's per-round table (FLBuffers::rtab): the sampled mask
};
// values cut at each end of K_r >= 1 sampled clients: median (K_r - 1) / 2, trimmed mean
// floor(beta K_r) in double, never more than the median's (fedmi/fl/aggregate.py trim_count)
__host__ __device__ inline int fl_robust_trim(int kind, double beta, int kr) {
    const int med = (kr - 1) / 2;
    if (kind == FL_ROBUST_MEDIAN) return med;
    const int t = (int)(beta * (double)kr);
    return t < med ? t : med;
}

// Multi-Krum screening (fl_screen.hip; Blanchard et al. 2017): parameters of the per-round pairwise
// distance and select launches, passed to those kernels alone.  Of the round's K_r sampled clients
// (rtab mask) the min(m, K_r - f) with the smallest sum of their K_r - f - 2 nearest squared
// whole-model distances are kept; fl_robust then aggregates over the kept set (its `keep` argument).
#define FL_SCREEN_MAX_K 64           // width of the rtab mask; one lane per client in the select kernel
// client pairs per workgroup of the distance kernel, tile x tile (the matrix is the same bits at every
// size).  Measured on the 14-50-200-2 image (profiles/screen_trace.jsonl): 1 / 2 / 4 take 10.1 / 11.9 /
// 22.2 us at K = 4, 10.4 / 12.0 / 22.6 us at K = 8 and 26.0 / 19.4-19.8 / 26.0 us at K = 64
__host__ __device__ constexpr int fl_screen_tile(int K) { return K <= 8 ? 1 : 2; }
struct FLScreen {
    int K;               // sources, 1 .. FL_SCREEN_MAX_K (source k is client k)
    int f;               // Byzantine clients assumed, >= 0
    int m;               // clients kept, >= 1; 0: K_r - f
    int max_rounds;      // rounds of rtab / entries of the kept-mask history; rounds past it are not live
    const float* rtab;   // a client's per-round table (FLBuffers::rtab): the sampled mask
};

// Geometric-median aggregation (fl_geomed.hip; Pillutla et al. 2022, RFA): parameters of the per-round
// smoothed-Weiszfeld launches, passed to those kernels alone.  From the coordinate-wise median of the
// round's sampled clients (rtab mask), T times: squared whole-model distances d_i to the estimate,
// weights 1 / max(nu, sqrt(d_i)) over the clients with d_i < +inf, the weighted combine.
#define FL_GEOMED_MAX_K 64           // width of the rtab mask
#define FL_GEOMED_MAX_ITERS 32
#define FL_GEOMED_THREADS 256        // floats of the image per workgroup: part of d_i's summation order
// one iteration's record in the caller's scratch, floats: [0, 64) the weights b_i the iteration combined
// with, [64, 128) the distances d_i it measured, [128, 130) the mask of the clients it combined (two
// 32-bit halves; 0: it kept the coordinate-wise median)
#define FL_GEOMED_SLOT 192
struct FLGeomed {
    int K;               // sources, 1 .. FL_GEOMED_MAX_K (source k is client k)
    int max_rounds;      // rounds of rtab; rounds past it are not live
    const float* rtab;   // a client's per-round table (FLBuffers::rtab): the sampled mask
    int T;               // Weiszfeld iterations, 1 .. FL_GEOMED_MAX_ITERS
    float nu;            // smoothing: lower bound of a distance in a weight, > 0
};
__host__ __device__ constexpr int fl_geomed_blocks(int Pimg) {
    return (Pimg + FL_GEOMED_THREADS - 1) / FL_GEOMED_THREADS;
}
// floats of scratch the launches need: two sets of per-workgroup distance partials (64 per workgroup),
// then T iteration records
__host__ __device__ constexpr long long fl_geomed_scratch_floats(int Pimg, int T) {
    return 2ll * fl_geomed_blocks(Pimg) * FL_GEOMED_MAX_K + (long long)T * FL_GEOMED_SLOT;
}

// Secure aggregation (fl_secagg.hip; Bonawitz et al. 2017, the arithmetic only): parameters of the
// per-round mask and open launches, passed to those kernels alone.  A sampled client's contribution c
// becomes q = clamp(rint(c 2^bits), -L, L), L = (2^31 - 1) / K_r, plus / minus the pair masks
// m(a, b)[p] = word p % 4 of Philox4x32-10 at counter (p / 4, round, 64 a + b, FL_SECAGG_STREAM) under
// (key0, key1), mod 2^32; the open sums the sampled clients' words and scales by 2^-bits.
#define FL_SECAGG_STREAM 0x47414353u  // distinct from the DP noise stream 0x46454450 (fl_dp.hip)
#define FL_SECAGG_MAX_K 64            // width of the rtab mask
#define FL_SECAGG_MIN_BITS 8
#define FL_SECAGG_MAX_BITS 30
struct FLSecAgg {
    int bits;            // fractional bits F, FL_SECAGG_MIN_BITS .. FL_SECAGG_MAX_BITS
    int K;               // open: sources, 1 .. FL_SECAGG_MAX_K (source k is client k)
    int first_client;    // mask: client index of the launch's first buffer
    int max_rounds;      // rounds of rtab / entries of a clamp history; rounds past it are not live
    uint32_t key0, key1; // mask: Philox key, the group's 64-bit seed, low and high word
    float scale;         // 2^bits, 2^-bits: filled in by the launchers
    float inv_scale;
    const float* rtab;   // a client's per-round table (FLBuffers::rtab): the sampled mask
};

// Byzantine attack models (fl_attack.hip; fedmi/fl/attack.py is the specification): parameters of the
// per-round launch that rewrites the contributions of the bad sampled clients in place, before the screen,
// the robust rule, the secure-aggregation mask and the sum.  With S_r the round's sampled clients (rtab
// mask), B_r = S_r & bad, H_r = S_r & ~bad, w_j client j's FedAvg weight (wtab row of the round; null: 1),
// x the image the round trained from and m_j = div(c_j, w_j), every k in B_r gets c_k = mul(w_k, a_k) on
// the real parameters:
//   FL_ATTACK_SIGN_FLIP : a_k = sub(x, mul(scale, sub(m_k, x)))
//   FL_ATTACK_GAUSS     : a_k = add(m_k, mul(scale, n_k)), n_k: dense parameter p takes lane p % 4 of the
//                         Box-Muller pairs of Philox4x32-10 at counter (p / 4, round, k, FL_ATTACK_STREAM)
//   FL_ATTACK_ALIE      : a_k = sub(mu, mul(z, sqrt(var))), mu / var the mean and the (|H_r| - 1)-normalised
//                         variance of the m_j over H_r (var = 0 for |H_r| = 1)  (Baruch et al. 2019)
//   FL_ATTACK_IPM       : a_k = sub(x, mul(scale, sub(mu, x)))                   (Xie et al. 2020)
// The kinds' values are their indices in fedmi/fl/attack.py ATTACKS.
#define FL_ATTACK_SIGN_FLIP 1
#define FL_ATTACK_GAUSS 2
#define FL_ATTACK_ALIE 3
#define FL_ATTACK_IPM 4
#define FL_ATTACK_MAX_K 64            // width of the rtab mask
#define FL_ATTACK_STREAM 0x4B435441u  // distinct from the DP noise stream 0x46454450 (fl_dp.hip), FL_QSGD_STREAM,
                                      // FL_RANDK_STREAM and FL_SECAGG_STREAM
struct FLAttack {
    int kind;                 // FL_ATTACK_*
    int K;                    // buffers, 1 .. FL_ATTACK_MAX_K (buffer k is client k)
    int max_rounds;           // rounds of rtab / wtab; rounds past it are not live
    float scale;              // s of sign-flip, sigma of gauss, eps of ipm; finite, > 0
    float z;                  // alie
    uint32_t key0, key1;      // gauss: Philox key, the 64-bit attack seed, low and high word
    unsigned long long bad;   // bit k: client k is Byzantine
    const float* rtab;        // a client's per-round table (FLBuffers::rtab): the sampled mask
    const float* wtab;        // [max_rounds][K] fp32 FedAvg weights of the clients' buffers; null: all 1
};

// Held-out scoring of the round's aggregated model (fl_heldout.hip): parameters of the per-round row and
// fold launches, passed to those kernels alone, as FLDp is.  Every buffer is caller-owned.  A live
// round r leaves hist_cm[r] = the C x C confusion counts of the round's output image on the n held-out
// rows (true class major, first-maximum argmax) and hist_loss[r] = the fp32 SUM of the rows' softmax
// cross-entropies lse(z) - z[y]; the fp32 master image is read whatever the engine's operand type.
#define FL_HELDOUT_MAX_ROWS (1 << 24)  // counts stay exact where a caller holds them in fp32
#define FL_HELDOUT_FOLD_THREADS 1024
struct FLHeldout {
    const float* X;      // [n, dim0] row-major held-out rows
    const int* y;        // [n] labels in [0, C)
    int n;               // 1 .. FL_HELDOUT_MAX_ROWS
    int max_rounds;      // rows of hist_cm / hist_loss; rounds past it are not live
    int keep_best;       // 1: the fold keeps the image of the round with the smallest loss sum
    int* scratch;        // [ceil(n / R)][C * C + 1] per-workgroup partials: counts, then the loss sum's bits
    int* hist_cm;        // [max_rounds][C * C]
    float* hist_loss;    // [max_rounds] fp32 loss SUMS
    float* best_image;   // keep_best: [Pimg]
    float* best;         // keep_best: {best loss sum (starts at +inf), best round's index as int bits (starts at -1)}
};

struct PeerArgs;  // peer_device.h
struct PeerPack;
// Launchers (fl_kernels.hip). `pg` = image the round trains from (the previous round's
// all-reduced comm buffer), `comm` = buffer this round publishes into (Pimg + tail floats).
// `cm_out` = this rank's confusion slots of pg's tail (FL_EVAL_FUSED only).
hipError_t fl_launch_train(const MLPDesc& d, const FLConfig& c, const FLBuffers& b,
                           const float* pg, const FLState* st_in, FLState* st_out,
                           int local_step, hipStream_t s, int mode = FL_EVAL_CLASSIC,
                           float* cm_out = nullptr, int fold_mask = FL_FOLD_B, bool shape_spec = false);
// (fl_train_spec.hip: the fp32 train kernel specialised for the reference shape; `shape_spec` above
// lets fl_launch_train pick it where fl_train_spec_ok holds)
bool fl_train_spec_ok(const MLPDesc& d, const FLConfig& c, int mode);
hipError_t fl_launch_train_spec(const FLConfig& c, const FLBuffers& b, const float* pg, const FLState* st_in,
                                FLState* st_out, int local_step, hipStream_t s, int mode, float* cm_out,
                                int fold_mask);
hipError_t fl_set_lds_limit_spec(size_t bytes);
// `st` = state the step runs under; with `fold` (FL_EVAL_FUSED rounds, first local step) it
// is the previous round's state: every block folds pg's tail into it, block 0 writes the
// round's state to `st_out`.
hipError_t fl_launch_adam(const MLPDesc& d, const FLConfig& c, const FLBuffers& b,
                          const float* pin, const float* anchor, float* comm,
                          const FLState* st, int local_step, hipStream_t s,
                          const MLPDescB* e = nullptr, FLState* st_out = nullptr, int fold = 0,
                          int tail_a = 0, int fold_mask = FL_FOLD_B, const PeerArgs* peer = nullptr, int wx = 0,
                          int afold = 0, bool adam_spec = false, bool slab_blocked = false);
// (fl_adam_spec.hip: the Adam kernel specialised for the reference shape at R = 32, one client, no
// exchange, no lag region, no undo buffer; `adam_spec` above lets fl_launch_adam pick it where
// fl_adam_spec_ok holds.)  Its only kernel argument: what that kernel reads of FLConfig / FLBuffers
// and of the launch -- pointers first, then the launch and optimizer scalars, the early-stop
// scalars of the (out-of-line) metric fold last.  224 bytes, against 1016 of the generic kernel.
struct FlAdamSpecArgs {
    const float* pin;
    const float* anchor;
    float* comm;
    const FLState* st;
    float* slab;
    float* local;
    float* m;
    float* v;
    const float* sched;
    const float* rtab;
    char* pk_local;
    int* sat;
    unsigned long long* dbg;
    FLState* st_out;
    double* hist_global;
    double* hist_rank;
    float* hist_loss;
    int n_slabs, slab_stride, local_steps, max_rounds;
    int local_step, fold, tail_a, fold_mask;
    float inv_n, omb1, omb2, beta2f, eps, weight_decay, prox_mu;
    int es_enabled, patience, metric_mode;
    double atol, rtol;
};
bool fl_adam_spec_ok(const MLPDesc& d, const MLPDescB* e, const FLConfig& c, const FLBuffers& b);
hipError_t fl_launch_adam_spec(const FLConfig& c, const FLBuffers& b, const float* pin, const float* anchor,
                               float* comm, const FLState* st, int local_step, int pack, FLState* st_out, int fold,
                               int tail_a, int fold_mask, hipStream_t s, bool slab_blocked = false);
// (fl_adam_local.hip: the Adam kernel without the in-kernel exchange; fl_launch_adam picks it)
hipError_t fl_launch_adam_local(const MLPDesc& d, const FLConfig& c, const FLBuffers& b, const float* pin,
                                const float* anchor, float* comm, const FLState* st, int local_step,
                                const MLPDescB& e, int pack, FLState* st_out, int fold, int tail_a, int fold_mask,
                                hipStream_t s);
// (fl_adam_local.hip: the Adam kernel for exchanges on LL chunks)
hipError_t fl_launch_adam_ll(const MLPDesc& d, const FLConfig& c, const FLBuffers& b, const float* pin,
                             const float* anchor, float* comm, const FLState* st, int local_step, const MLPDescB& e,
                             int pack, FLState* st_out, int fold, int tail_a, int fold_mask, const PeerArgs& pa,
                             int xchg, int afold, hipStream_t s);
hipError_t fl_launch_eval(const MLPDesc& d, const FLConfig& c, const FLBuffers& b,
                          const float* params, float* comm, const FLState* st, hipStream_t s);
// (fl_dp.hip) clip + noise of the round whose last Adam kernel wrote state `st`: rewrites the
// first Pimg floats of `comm` from `local` and the round's input image `pg`
hipError_t fl_launch_dp(const MLPDesc& d, const FLDp& p, const float* local, const float* pg, float* comm,
                        const FLState* st, const float* rtab, hipStream_t s);
// (fl_compress.hip) compression of the round whose last Adam kernel wrote state `st`: rewrites the
// real parameters of the first Pimg floats of `comm` from `local`, the round's input image `pg` and
// the residual.  fl_set_lds_limit_compress: once per model before the first launch (dynamic LDS).
hipError_t fl_set_lds_limit_compress(const MLPDesc& d, int kind = FL_COMPRESS_TOPK);
hipError_t fl_launch_compress(const MLPDesc& d, const FLCompress& p, const float* local, const float* pg, float* comm,
                              const FLState* st, const float* rtab, hipStream_t s);
// (fl_server.hip) server-optimizer step of the round whose state is `st`: `x` = the image the round
// trained from, `a` = its aggregated image, replaced in place (first Pimg floats only) by the new
// global image.  `e` / `pk` (bf16 mode, else null): the same launch also writes the packed
// split-bf16 image of the result into `pk`.
hipError_t fl_launch_server(const MLPDesc& d, const FLServer& p, const float* x, float* a, const FLState* st,
                            const MLPDescB* e, char* pk, hipStream_t s);
// (fl_robust.hip) robust aggregate of the round whose state is `st`, over the K buffers of Pimg +
// `tails_len` floats named by the device pointer table `src`, written to the `n_dst` buffers named by
// the device pointer table `dst` (destinations may be sources).  Image: median / trimmed mean of the
// round's sampled clients, padding exact 0; tails, and the whole buffer of a round that is not live:
// the left fold in source order.  No per-round host argument: the launch is replayable.  `keep` (may
// be null): the kept-client mask of the round's screening (fl_screen.hip), ANDed into the sampled mask
// of a live round -- the rule then runs over the kept clients.
hipError_t fl_launch_robust(const MLPDesc& d, const FLRobust& p, const float* const* src, float* const* dst, int n_dst,
                            const FLState* st, int tails_len, hipStream_t s,
                            const unsigned long long* keep = nullptr);
// (fl_screen.hip) multi-Krum screening of the round whose state is `st`, over the K images named by the
// device pointer table `src`.  Dist: the K x K fp32 matrix of squared distances between the round's
// sampled clients into the caller-owned `dist` (both triangles, zero diagonal; entries of unsampled
// clients are unspecified); `tile` = client pairs per workgroup, tile x tile (1, 2, 4; 0: fl_screen_tile(K))
// -- the matrix does not depend on it.  Select: from `dist`, the kept-client mask into `*keep` and
// `hist[round]`.  A round that is not live writes nothing.  Both replayable.
hipError_t fl_launch_screen_dist(const MLPDesc& d, const FLScreen& p, const float* const* src, float* dist,
                                 const FLState* st, hipStream_t s, int tile = 0);
hipError_t fl_launch_screen_select(const FLScreen& p, const float* dist, unsigned long long* keep,
                                   unsigned long long* hist, const FLState* st, hipStream_t s);
// (fl_geomed.hip) geometric-median aggregate of the round whose state is `st`: the T + 1 launches of the
// smoothed Weiszfeld iteration over the K buffers of Pimg + tails_len floats named by `src`, the result
// into the n_dst buffers named by `dst` (they may be the sources).  `scratch`: fl_geomed_scratch_floats
// caller-owned floats; iteration t's record (FL_GEOMED_SLOT) lies at 2 * blocks * 64 + t * FL_GEOMED_SLOT.
// A round that is not live is the whole-buffer left fold and writes no scratch.  `keep` as fl_launch_robust's.
// No per-round host argument: the sequence is replayable.
hipError_t fl_launch_geomed(const MLPDesc& d, const FLGeomed& p, const float* const* src, float* const* dst, int n_dst,
                            const FLState* st, int tails_len, float* scratch, hipStream_t s,
                            const unsigned long long* keep = nullptr);
// (fl_attack.hip) the Byzantine clients' contributions of the round whose state is `st`: one launch rewrites,
// in place, the real parameters of the bad sampled ones among the K buffers named by the device table `bufs`
// (image padding, metric tails, honest and unsampled clients' buffers are never written; a round that is not
// live, one without a bad sampled client and, alie / ipm, one without an honest sampled client write
// nothing).  `x`: the image the round trained from.  No per-round host argument: the launch is replayable.
hipError_t fl_launch_attack(const MLPDesc& d, const FLAttack& p, float* const* bufs, const float* x,
                            const FLState* st, hipStream_t s);
// (fl_secagg.hip) secure aggregation of the round whose state is `st`.  Mask: quantises and pair-masks, in
// place, the real parameters of the `n` buffers named by the device pointer table `bufs` (clients
// first_client .. first_client + n - 1; unsampled ones and rounds that are not live are left alone);
// `clamp`: device table of the n clients' uint32 [max_rounds] clamp histories.  Open: over the K buffers
// of Pimg + `tails_len` floats named by `src`, written to the `n_dst` buffers named by `dst` (destinations
// may be sources).  Image: the scaled integer sum of the round's sampled clients, padding exact 0; tails,
// and the whole buffer of a round that is not live: the left fold in source order.  Both replayable.
hipError_t fl_launch_secagg_mask(const MLPDesc& d, const FLSecAgg& p, float* const* bufs, int n,
                                 uint32_t* const* clamp, const FLState* st, hipStream_t s);
hipError_t fl_launch_secagg_open(const MLPDesc& d, const FLSecAgg& p, const float* const* src, float* const* dst,
                                 int n_dst, const FLState* st, int tails_len, hipStream_t s);
// (fl_heldout.hip) held-out scoring of the round whose state is `st` and whose output image is `image`:
// the row launch (one workgroup per R = 16 or 32 held-out rows, partials into p.scratch) and the fold
// launch (one workgroup: round r's row of p.hist_cm / p.hist_loss, and with p.keep_best the best image).
// `d`: the model's descriptor built for R rows.  A round that is not live writes nothing.  No per-round
// host argument: both launches are replayable.  fl_set_lds_limit_heldout: once per model (dynamic LDS).
hipError_t fl_set_lds_limit_heldout(size_t bytes);
hipError_t fl_launch_heldout(const MLPDesc& d, int R, const FLHeldout& p, const float* image, const FLState* st,
                             hipStream_t s);
// ... and its row mode: the fp32 softmax of `params`' logits on rows [0, n) of X into proba[n][C] and / or
// their first-maximum argmax into pred[n] (either may be null, not both); ungated.
hipError_t fl_launch_heldout_predict(const MLPDesc& d, int R, const float* X, int n, const float* params,
                                     float* proba, int* pred, hipStream_t s);
// `prev_out` (may be null): the other parameter buffer -- the round before pg's output.  When
// the fold finds a late stop (FLState::late) pg's image is replaced by it.
hipError_t fl_launch_finalize(const MLPDesc& d, const FLConfig& c, const FLBuffers& b,
                              float* pg, const FLState* st_in, FLState* st_out,
                              hipStream_t s, int mask = FL_FOLD_B, const float* prev_out = nullptr);
// bf16-operand variants (split-bf16 forward, bf16 backward, fp32 accumulate, fp32 master
// weights / slab / Adam state).
hipError_t fl_launch_train_bf16(const MLPDesc& d, const MLPDescB& e, const FLConfig& c, const FLBuffers& b,
                                const float* pg, const FLState* st_in, FLState* st_out, int local_step,
                                hipStream_t s, bool stage_local = false, int mode = FL_EVAL_CLASSIC,
                                float* cm_out = nullptr, int fold_mask = FL_FOLD_B, bool shape_spec = false,
                                bool slab_blocked = false, bool epi_exchange = false);
// (fl_train_bf16_spec.hip: the train kernel specialised for the reference shape, fl_layout.h FlRefShape.
// `shape_spec` above lets fl_launch_train_bf16 pick it where fl_train_bf16_spec_ok holds: descriptors
// byte-equal to the compile-time ones, and a round kind that is instantiated)
// `slab_blocked` (FLEngine's flag, the same value to fl_launch_adam): the fp16 slab row is the blocked
// one of fl_layout.h (FlSlabBlk), which only the specialised train / Adam pair writes and reads; a
// launch that would take another kernel fails instead, so a mixed pair never runs.
// `epi_exchange` (FLEngine's flag): the specialised kernel's hidden-layer forward and dgrad epilogues are
// the exchanged ones (fl_layout.h fl_epi_*: transposed tiles, 8-byte LDS stores; the same LDS bytes); the
// generic kernels have no such form and ignore it.
bool fl_train_bf16_spec_ok(const MLPDesc& d, const MLPDescB& e, const FLConfig& c, int mode);
hipError_t fl_launch_train_bf16_spec(const FLConfig& c, const FLBuffers& b, const float* pg, const FLState* st_in,
                                     FLState* st_out, int local_step, hipStream_t s, bool stage_local, int mode,
                                     float* cm_out, int fold_mask, bool slab_blocked = false,
                                     bool epi_exchange = false);
hipError_t fl_set_lds_limit_bf16_spec(size_t bytes);
hipError_t fl_launch_eval_bf16(const MLPDesc& d, const MLPDescB& e, const FLConfig& c, const FLBuffers& b,
                               const float* params, float* comm, const FLState* st, hipStream_t s);
hipError_t fl_set_lds_limit_bf16(size_t bytes);
// fp32 parameter image -> packed bf16 LDS-layout parameter region (MLPDescB)
// Local evaluation + FedAvg in one kernel (world > 1 with the one-shot xGMI all-reduce,
// peer_device.h): the all-reduce of the call described by `a` runs in extra blocks beside
// the evaluation of `params` into this rank's tail slot of `comm` (the call's send buffer).
hipError_t fl_launch_eval_fedavg(const MLPDesc& d, const FLConfig& c, const FLBuffers& b, const float* params,
                                 float* comm, const FLState* st, const PeerArgs& a, const PeerPack& pk,
                                 hipStream_t s);
hipError_t fl_launch_eval_fedavg_bf16(const MLPDesc& d, const MLPDescB& e, const FLConfig& c, const FLBuffers& b,
                                      const float* params, float* comm, const FLState* st, const PeerArgs& a,
                                      const PeerPack& pk, hipStream_t s);
hipError_t fl_launch_pack_bf16(const MLPDesc& d, const MLPDescB& e, const float* params, char* out, hipStream_t s);
// Batched launches of K trials (FLTrialDesc table `T`, K = gridDim.y): the same kernels, every
// pointer argument a selector into the trial's bases.  `cm` of the train launch and `comm` of
// the eval launch follow the single-trial launchers (the eval's confusion slots are derived
// from `comm` per trial).
hipError_t fl_launch_train_batch(const MLPDesc& d, int R, int n_slabs, const FLTrialDesc* T, int K, FLSel pg,
                                 FLSel si, FLSel so, int ls, int mode, FLSel cm, int fold_mask, hipStream_t s);
hipError_t fl_launch_train_bf16_batch(const MLPDesc& d, const MLPDescB& e, int R, int n_slabs, const FLTrialDesc* T,
                                      int K, FLSel pg, FLSel si, FLSel so, int ls, int stage_local, int mode, FLSel cm,
                                      int fold_mask, hipStream_t s, int plain = 0);
hipError_t fl_launch_adam_batch(const MLPDesc& d, const MLPDescB* e, const FLTrialDesc* T, int K, FLSel pin,
                                FLSel anchor, FLSel comm, FLSel st, int local_step, FLSel st_out, int fold, int tail_a,
                                int fold_mask, hipStream_t s);
hipError_t fl_launch_eval_batch(const MLPDesc& d, int R, int n_rows, const FLTrialDesc* T, int K, FLSel params,
                                FLSel comm, FLSel st, hipStream_t s);
hipError_t fl_launch_eval_bf16_batch(const MLPDesc& d, const MLPDescB& e, int R, int n_rows, const FLTrialDesc* T,
                                     int K, FLSel params, FLSel comm, FLSel st, hipStream_t s);
hipError_t fl_launch_pack_bf16_batch(const MLPDesc& d, const MLPDescB& e, const FLTrialDesc* T, int K, FLSel params,
                                     FLSel out, hipStream_t s);
hipError_t fl_launch_finalize_batch(const MLPDesc& d, const FLTrialDesc* T, int K, FLSel pg, FLSel si, FLSel so,
                                    int mask, hipStream_t s);
// Stand-alone forward + confusion on an arbitrary row set (held-out evaluation).
hipError_t fl_launch_confusion(const MLPDesc& d, int R, const float* X, const int* y, int n_rows,
                               const float* params, float* cm_out, hipStream_t s);
// Fill a device shard with synthetic income-shaped rows (Philox4x32-10).
hipError_t fl_launch_synth(float* X, int* y, long long n_rows, int n_features,
                           unsigned long long seed, unsigned long long row_offset,
                           const float* teacher_w1, const float* teacher_w2, int teacher_hidden,
                           hipStream_t s, float label_noise = 0.f);
// Hold stream `s` for `us` microseconds (one sleeping wave; FLEngine::trace).
hipError_t fl_launch_gate(double us, hipStream_t s);
