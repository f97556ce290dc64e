// Host-side layout arithmetic of the fused round kernels: the fp32 parameter image and LDS
// layout (MLPDesc) and the bf16 LDS layouts of the train / evaluation kernels (MLPDescB).
// Header-only and free of HIP runtime calls, so the same code the engine uses is compiled into
// a host test binary with AddressSanitizer + UBSan (tests/native/test_layout.cpp) that sweeps
// model shapes and checks every region the kernels index for bounds, overlap and alignment.
#pragma once
#include <algorithm>
#include <cstring>

#include "fl_common.h"

// Activation row stride: roundup16(dim) + 4 floats (16-byte aligned rows, 4 mod 8: with the
// chunk swizzle of fl_kernels.hip (fl_swz) the b128 / b32 MFMA operand patterns are
// bank-conflict free).
constexpr int fl_pick_ld(int dim) { return ((dim + 15) & ~15) + 4; }

// dims[0..L]: features, hidden sizes, classes.  Fills the dense / image offsets and the fp32
// kernels' LDS layout (floats) for R rows per workgroup.
constexpr void fl_build_fp32_layout(const int* dims, int L, int R, MLPDesc* d) {
    *d = MLPDesc{};
    d->L = L;
    int off = 0;
    for (int l = 0; l <= L; ++l) d->dim[l] = dims[l];
    for (int l = 0; l < L; ++l) {
        d->w_off[l] = off;
        off += dims[l] * dims[l + 1];
        d->b_off[l] = off;
        off += dims[l + 1];
    }
    d->P = off;
    // parameter image (fl_common.h): per layer [wrows(N)][ldw(K)] then bias[roundup16(N)]
    int io = 0;
    for (int l = 0; l < L; ++l) {
        d->iw_off[l] = io;
        io += fl_wrows(dims[l + 1]) * fl_ldw(dims[l]);
        d->ib_off[l] = io;
        io += (dims[l + 1] + 15) & ~15;
    }
    d->Pimg = (io + 3) & ~3;
    int lds = 0;
    for (int l = 0; l <= L; ++l) {
        d->ld[l] = fl_pick_ld(dims[l]);
        d->act_off[l] = lds;
        lds += R * d->ld[l];
        lds = (lds + 3) & ~3;
    }
    for (int l = 1; l < L; ++l) {  // backward deltas of the hidden layers
        d->dlt_off[l] = lds;
        lds += R * d->ld[l];
        lds = (lds + 3) & ~3;
    }
    d->cm_off = lds;  // fused evaluation's confusion counters (FL_CM_INTS ints)
    lds += FL_CM_INTS;
    d->img_lds = lds;
    lds += d->Pimg;
    d->lds_floats = lds;
}

// Lagged rounds (FL_EVAL_LAGGED) score the previous round's local model in registers
// (fl_kernels_bf16.hip score_rows_regs) when: one or two hidden layers; the register operands
// fit (features <= 32, with two hidden layers the first <= 64 wide); C <= FL_LAG_MAX_C; the
// logits' K split leaves each upper scoring wave at most FL_LAG_PARTS partials; the training
// forward pass fits the first FL_WAVES - FL_LAG_SPR R/16 waves (hidden tiles are strided over them; the
// logits layer's split K loop and its partial sum must fit them as they are), so the last
// FL_LAG_SPR R/16 waves -- FL_LAG_SPR per 16 rows -- score while the others train; and the LDS holds the
// partials beside the layout.  Otherwise the scoring pass runs before the training pass on the
// whole workgroup.
constexpr int fl_lag_reg_static_bytes(int R) { return (R / 16) * ((FL_LAG_SPR - 1) * FL_LAG_PARTS * 16 * 16 + 16); }
constexpr bool fl_lag_reg_ok(const MLPDesc& d, const MLPDescB& e, int R) {
    const int L = d.L, C = d.dim[L];
    const int nw = FL_WAVES - FL_LAG_SPR * (R / 16);
    if ((R != 16 && R != 32) || nw < 1 || (L != 2 && L != 3) || C > FL_LAG_MAX_C) return false;
    if (e.kp[0] > 32 || (L == 3 && e.kp[1] > 64)) return false;
    const int G = e.head_split;
    if (G > nw) return false;
    for (int j = 1; j < FL_LAG_SPR; ++j)
        if (fl_lag_w(G, j + 1) - fl_lag_w(G, j) > FL_LAG_PARTS) return false;
    if (R * C > nw * 64) return false;  // the logits' partial sums (fwd_head_split_bf16) run on thread < R*C
    // the partials ride in static LDS beside the dynamic layout (FL_LDS_DYNAMIC_MAX keeps 2 KB for
    // the kernels' own small statics; ~256 B are taken)
    return e.lds_bytes + fl_lag_reg_static_bytes(R) + 256 <= 160 * 1024;
}

// bf16 LDS layouts (fl_common.h MLPDescB), byte offsets, 16-byte aligned pieces: `e` for the
// train kernel, `ev` for the evaluation kernels (forward pass only), at bank layout `level`.
constexpr void fl_build_bf16_layout_level(const MLPDesc& d, int R, int level, MLPDescB* e_out, MLPDescB* ev_out) {
    MLPDescB e{}, ev{};
    const int L = d.L;
    e.level = level;
    e.wgap = level == 2 ? 128 : 0;
    e.wxor = level == 2 ? 0 : 1;
    for (int l = 0; l <= L; ++l) {
        e.kp[l] = (d.dim[l] + 31) & ~31;
        e.lda[l] = e.kp[l] + (level >= 1 ? 16 : 8);
        if (l < L) e.ldw[l] = e.kp[l] + (level == 2 ? 16 : 8);
    }
    int off = 0;
    auto take = [&](int bytes) { const int o = off; off += (bytes + 15) & ~15; return o; };
    for (int l = 0; l < L; ++l) e.act_off[l] = take(R * e.lda[l] * 2);
    for (int l = 1; l <= L; ++l) e.dlt_off[l] = take(R * e.lda[l] * 2);
    e.logit_off = take(R * FL_LOGIT_LD * 4);
    e.cm_off = take(FL_CM_INTS * 4);
    // split-bf16 forward: lo parts of the layer inputs -- X in its own buffer, the hidden
    // activations in the delta buffers (same [R][lda] shape, free until the backward pass)
    e.alo_off[0] = take(R * e.lda[0] * 2);
    for (int l = 1; l < L; ++l) e.alo_off[l] = e.dlt_off[l];
    // parameter region: W hi images, biases, W lo images (each W size is a multiple of 16
    // bytes, so the lo images sit at one constant offset from their hi images)
    e.param_off = off;
    for (int l = 0; l < L; ++l) e.w_off[l] = take(fl_wrow(e.kp[l + 1], e.ldw[l], e.wgap));
    for (int l = 0; l < L; ++l) e.bias_off[l] = take(e.kp[l + 1] * 4);
    e.wlo_delta = off - e.w_off[0];
    for (int l = 0; l < L; ++l) take(fl_wrow(e.kp[l + 1], e.ldw[l], e.wgap));
    e.param_bytes = off - e.param_off;
    e.lds_bytes = off;
    e.item_base[0] = 0;
    for (int l = 0; l < L; ++l) e.item_base[l + 1] = e.item_base[l] + e.kp[l + 1] * (e.kp[l] >> 3);
    // Evaluation kernels run the forward pass only: their layout has no delta buffers, so the
    // lo parts of the hidden activations get buffers of their own.
    ev = e;
    off = 0;
    for (int l = 0; l < L; ++l) ev.act_off[l] = take(R * e.lda[l] * 2);
    for (int l = 1; l <= L; ++l) ev.dlt_off[l] = -1;
    ev.logit_off = take(R * FL_LOGIT_LD * 4);
    ev.cm_off = take(FL_CM_INTS * 4);
    for (int l = 0; l < L; ++l) ev.alo_off[l] = take(R * e.lda[l] * 2);
    ev.param_off = off;
    for (int l = 0; l < L; ++l) {
        ev.w_off[l] = e.w_off[l] - e.param_off + ev.param_off;
        ev.bias_off[l] = e.bias_off[l] - e.param_off + ev.param_off;
    }
    ev.lds_bytes = ev.param_off + e.param_bytes;
    // Logits layer (one 16-column tile): its K loop is split over up to 16 waves (fixed-order
    // sum of the partial logits) instead of one wave's chain of kp/32 steps, as far as LDS room
    // allows; the same split in both layouts, so training, fused and classic evaluation see
    // bit-identical logits.
    const int C = d.dim[L];
    const int part1 = R * C * 4;
    const int ksteps = e.kp[L - 1] >> 5;
    const int room = (int)FL_LDS_DYNAMIC_MAX - std::max(e.lds_bytes, ev.lds_bytes) - 16;
    int G = std::min(std::min(ksteps, 16), std::max(1, room / part1));
    if (G < 2) G = 1;
    e.head_split = ev.head_split = G;
    if (G > 1) {
        e.part_off = e.lds_bytes;
        e.lds_bytes += (G * part1 + 15) & ~15;
        ev.part_off = ev.lds_bytes;
        ev.lds_bytes += (G * part1 + 15) & ~15;
    }
    e.lag_reg = ev.lag_reg = fl_lag_reg_ok(d, e, R) ? 1 : 0;
    *e_out = e;
    *ev_out = ev;
}

// The most conflict-free level whose train and evaluation layouts fit the CU's LDS (level 0
// when none fits: the engine then refuses this R).
constexpr void fl_build_bf16_layout(const MLPDesc& d, int R, MLPDescB* e_out, MLPDescB* ev_out) {
    for (int level = 2; level >= 0; --level) {
        fl_build_bf16_layout_level(d, R, level, e_out, ev_out);
        if (std::max(e_out->lds_bytes, ev_out->lds_bytes) <= (int)FL_LDS_DYNAMIC_MAX) return;
    }
}

// The reference shape -- BASELINE's 14-50-200-2 income MLP -- with its layouts at R rows per
// workgroup as constants, from the functions above: what the engine computes at run time for this
// shape, evaluated by the compiler.  The shape-specialised train kernels take their strides, offsets
// and trip counts from here and no descriptor arguments; a launcher may pick them only for run-time
// descriptors that are byte-equal to these (fl_ref_shape_match; both structs are all int, no padding).
struct FlRefLayouts {
    MLPDesc d;
    MLPDescB e, ev;
};
constexpr FlRefLayouts fl_ref_layouts(int R) {
    constexpr int dims[4] = {14, 50, 200, 2};
    FlRefLayouts s{};
    fl_build_fp32_layout(dims, 3, R, &s.d);
    fl_build_bf16_layout(s.d, R, &s.e, &s.ev);
    return s;
}
template <int R>
struct FlRefShape {
    static constexpr FlRefLayouts all = fl_ref_layouts(R);
    static constexpr MLPDesc d = all.d;
    static constexpr MLPDescB e = all.e, ev = all.ev;
};
template <int R>
inline bool fl_ref_shape_match(const MLPDesc& d, const MLPDescB& e) {
    const MLPDesc rd = FlRefShape<R>::d;  // copies: the comparison needs no definition of the members
    const MLPDescB re = FlRefShape<R>::e;
    return std::memcmp(&d, &rd, sizeof(d)) == 0 && std::memcmp(&e, &re, sizeof(e)) == 0;
}

// Blocked fp16 gradient-slab row (reference shape, R = 32: the specialised bf16 train kernel writes it,
// the specialised Adam kernel reads it; every other kernel pair keeps the dense [o][K] order).  The
// weight gradient of layer l (K inputs, N outputs) is stored as blocks of 16 inputs, [it][o][w]:
// block `it` holds inputs 16 it .. 16 it + w - 1 of every output, w = min(16, K - 16 it) rounded up to
// a multiple of 4, so element (o, i) sits at fl_slab_blk_off(l, it) + o w + i % 16.  Every block starts
// on a multiple of 32 halves (64 bytes), and a 16 x 16 wgrad tile whose lanes hold 4 consecutive
// inputs of one output (fl_kernels_bf16.hip wgrad_layer_bf16) is one contiguous run of at most 512
// bytes, one aligned 8-byte store per lane.  Columns i >= K inside a block are pads: the train kernel
// writes them on every launch (exact zeros: the padded activation columns are zero), no parameter
// maps to them.  The bias gradients follow in dense order; the row's P halves are rounded up to a
// multiple of 8 with zeros (the Adam kernel reads 16-byte chunks), and the loss partial stays the
// fp32 at float index P of the row, as in the dense row.
struct FlSlabBlk {
    int lay_off[FL_MAX_LAYERS];  // first block of layer l's weight gradient (halves)
    int bstride[FL_MAX_LAYERS];  // halves from one block of the layer to the next: roundup32(16 N)
    int b_off[FL_MAX_LAYERS];    // bias gradient of layer l
    int P;                       // halves of the row that hold gradients (pads included)
    int Pz;                      // P rounded up to a multiple of 8: [P, Pz) is zero-filled
};
__host__ __device__ constexpr int fl_slab_blk_w(int K, int it) { return ((K - 16 * it < 16 ? K - 16 * it : 16) + 3) & ~3; }
__host__ __device__ constexpr int fl_slab_blk_off(const FlSlabBlk& s, int l, int it) { return s.lay_off[l] + it * s.bstride[l]; }
constexpr FlSlabBlk fl_slab_blk_build(const MLPDesc& d) {
    FlSlabBlk s{};
    int off = 0;
    for (int l = 0; l < d.L; ++l) {
        const int K = d.dim[l], N = d.dim[l + 1], itiles = (K + 15) >> 4;
        off = (off + 31) & ~31;
        s.lay_off[l] = off;
        s.bstride[l] = (16 * N + 31) & ~31;
        off += (itiles - 1) * s.bstride[l] + N * fl_slab_blk_w(K, itiles - 1);
    }
    off = (off + 7) & ~7;
    for (int l = 0; l < d.L; ++l) {
        s.b_off[l] = off;
        off += d.dim[l + 1];
    }
    s.P = off;
    s.Pz = (off + 7) & ~7;
    return s;
}
// The row is gap-free when every block ends where the next one starts (each position below P is
// then a gradient or a pad column, all of them written by the train kernel).
constexpr bool fl_slab_blk_gapfree(const MLPDesc& d, const FlSlabBlk& s) {
    for (int l = 0; l < d.L; ++l) {
        const int K = d.dim[l], N = d.dim[l + 1], itiles = (K + 15) >> 4;
        if (itiles > 1 && s.bstride[l] != 16 * N) return false;
        const int end = fl_slab_blk_off(s, l, itiles - 1) + N * fl_slab_blk_w(K, itiles - 1);
        if (end != (l + 1 < d.L ? s.lay_off[l + 1] : s.b_off[0])) return false;
    }
    return true;
}
// Dense parameter index -> position in the blocked row.
__host__ __device__ constexpr int fl_slab_blk_pos(const MLPDesc& d, const FlSlabBlk& s, int di) {
    int l = 0;
    for (int t = 1; t < d.L; ++t)
        if (di >= d.w_off[t]) l = t;
    if (di >= d.b_off[l]) return s.b_off[l] + (di - d.b_off[l]);
    const int K = d.dim[l], q = di - d.w_off[l];
    const int o = q / K, i = q - o * K, it = i >> 4;
    return fl_slab_blk_off(s, l, it) + o * fl_slab_blk_w(K, it) + (i & 15);
}
// Position in the blocked row -> dense parameter index, -1 for a pad (the inverse of fl_slab_blk_pos;
// one arm per layer, so under constant descriptors every division is by a constant).
__host__ __device__ constexpr int fl_slab_blk_dense(const MLPDesc& d, const FlSlabBlk& s, int pos) {
    if (pos < 0 || pos >= s.P) return -1;
    int di = -1;
#pragma unroll
    for (int l = 0; l < FL_MAX_LAYERS; ++l) {
        if (l >= d.L) continue;
        const int K = d.dim[l], N = d.dim[l + 1], itiles = (K + 15) >> 4;
        if (pos >= s.b_off[l] && pos < s.b_off[l] + N) di = d.b_off[l] + (pos - s.b_off[l]);
        const int q = pos - s.lay_off[l];
        if (q < 0 || q >= (itiles - 1) * s.bstride[l] + N * fl_slab_blk_w(K, itiles - 1)) continue;
        int it = q / s.bstride[l];
        it = it < itiles ? it : itiles - 1;
        const int r = q - it * s.bstride[l], w = fl_slab_blk_w(K, it);
        const int o = r / w, i = 16 * it + (r - o * w);
        if (o < N && i < K) di = d.w_off[l] + o * K + i;
    }
    return di;
}
template <int R>
struct FlRefSlabBlk {
    static constexpr FlSlabBlk s = fl_slab_blk_build(FlRefShape<R>::d);
    static_assert(fl_slab_blk_gapfree(FlRefShape<R>::d, s), "reference shape: the blocked slab row has no gaps");
};

// Exchanged epilogues of the specialised bf16 train kernel (SP::kEpiExchange; fl_kernels_bf16.hip
// fwd_layer_bf16, dgrad_layer_bf16).  With the two MFMA operands exchanged a 16 x 16 tile comes out
// transposed -- same products at the same k positions, same accumulator bits -- so accumulator j of lane
// `lane` (lr = lane & 15, lg = lane >> 4) is one row's value at 4 consecutive columns instead of one
// column's at 4 rows, and the lane's 4 bf16 results leave as one aligned 8-byte LDS store.  Row tile rt:
// the lane's row.  Forward column tile nt: lane lr loads W row nt*16 + fl_fwd_col(lr), so accumulator
// 4 lg + j is column nt*16 + fl_fwd_col(4 lg + j) = nt*16 + 4 ((lg + 1) & 3) + j.  dgrad item `it`: the
// transposed W reads give lane lr feature it*16 + lr, accumulator 4 lg + j is feature it*16 + 4 lg + j.
// fl_epi_off: byte offset of (row, col) in a bf16 buffer of row stride `lda` elements (act_l, alo_l, D_l).
__host__ __device__ constexpr int fl_epi_row(int rt, int lane) { return rt * 16 + (lane & 15); }
__host__ __device__ constexpr int fl_epi_fwd_col(int nt, int lane, int j) { return nt * 16 + 4 * (((lane >> 4) + 1) & 3) + j; }
__host__ __device__ constexpr int fl_epi_dgrad_col(int it, int lane, int j) { return it * 16 + 4 * (lane >> 4) + j; }
__host__ __device__ constexpr int fl_epi_off(int row, int col, int lda) { return (row * lda + col) * 2; }

// Shape policies of the train kernels' device functions (template parameter SP): where a function
// takes its descriptors from.  FlShapeDyn: the by-value kernel arguments, as passed.  FlShapeRef<R>:
// the reference shape's constants -- the arguments are ignored, every stride, offset and trip count
// folds at compile time (kStatic: the functions then also unroll their layer, K and tile loops).
// A function binds its descriptors with FL_SHAPE_D / FL_SHAPE_E (name, argument): a reference bound
// by a constant-condition select -- under FlShapeDyn to the argument itself, exactly as without a
// policy; under FlShapeRef to a function-local constexpr copy of the constants, which the compiler
// folds (a load from the class-scope object is not folded in device code: such objects are
// constant-memory symbols the host may overwrite).
// kSlabBlocked (FlShapeRef<R, true>, bf16 train kernel only): the fp16 slab row is the blocked one
// above (FlRefSlabBlk<R>) instead of the dense row.
// kEpiExchange (FlShapeRef<R, BLK, true>, bf16 train kernel only): the hidden layers' forward tiles and
// the dgrad tiles come out transposed and leave as 8-byte LDS stores (fl_epi_* above).
struct FlShapeDyn {
    static constexpr bool kStatic = false;
    static constexpr bool kSlabBlocked = false;
    static constexpr bool kEpiExchange = false;
    static constexpr const MLPDesc* pd = nullptr;
    static constexpr const MLPDescB* pe = nullptr;
    static constexpr const FlSlabBlk* ps = nullptr;
};
template <int R, bool BLK = false, bool EPI = false>
struct FlShapeRef {
    static constexpr bool kStatic = true;
    static constexpr bool kSlabBlocked = BLK;
    static constexpr bool kEpiExchange = EPI;
    static constexpr const FlSlabBlk* ps = &FlRefSlabBlk<R>::s;
    static constexpr const MLPDesc* pd = &FlRefShape<R>::d;
    static constexpr const MLPDescB* pe = &FlRefShape<R>::e;
};
#define FL_SHAPE_D(SP, name, arg)                                          \
    constexpr MLPDesc name##_const = SP::kStatic ? *SP::pd : MLPDesc{};    \
    const MLPDesc& name = SP::kStatic ? name##_const : (arg)
#define FL_SHAPE_E(SP, name, arg)                                          \
    constexpr MLPDescB name##_const = SP::kStatic ? *SP::pe : MLPDescB{};  \
    const MLPDescB& name = SP::kStatic ? name##_const : (arg)
