// The blocked fp16 gradient-slab row of the reference 14-50-200-2 MLP (fl_layout.h FlSlabBlk): the map
// from dense parameter index to row position (what the train kernel stores to and slab_partials gathers
// through) and its inverse (what the specialised Adam kernel evaluates per lane), against the layout's
// definition -- blocks of 16 inputs [it][o][w], biases behind them in dense order.  Injective, every
// non-pad position hit exactly once, pads exactly the i >= K columns, blocks 64-byte aligned, every
// lane's 4-value store of a wgrad tile 8-byte aligned and inside its block, the tiles of a layer
// covering its blocks exactly once, and the row length the engine allocates.
// Stand-alone host program (built with AddressSanitizer + UBSan by tests/test_native_slab_map.py).
#include <cstdio>
#include <vector>

#include "fl_layout.h"

static_assert(FlRefSlabBlk<32>::s.lay_off[0] == 0 && FlRefSlabBlk<32>::s.lay_off[1] == 800, "layer 0: one block of 50 x 16");
static_assert(FlRefSlabBlk<32>::s.lay_off[2] == 800 + 3 * 3200 + 800, "layer 1: three blocks of 200 x 16, one of 200 x 4");
static_assert(FlRefSlabBlk<32>::s.b_off[0] == 11200 + 12 * 32 + 16, "head: twelve blocks of 2 x 16, one of 2 x 8");
static_assert(fl_slab_blk_dense(FlRefShape<32>::d, FlRefSlabBlk<32>::s, 14) == -1, "first pad column");
static_assert(fl_slab_blk_dense(FlRefShape<32>::d, FlRefSlabBlk<32>::s, 16) == 14, "second output's first input");

static int failures = 0;
static void fail(const char* what, int at, int a, int b) {
    if (++failures <= 20) std::printf("%d: %s %d != %d\n", at, what, a, b);
}

int main() {
    const int dims[4] = {14, 50, 200, 2};
    MLPDesc d;
    fl_build_fp32_layout(dims, 3, 32, &d);
    const FlSlabBlk s = fl_slab_blk_build(d);
    const FlSlabBlk cs = FlRefSlabBlk<32>::s;
    const MLPDesc cd = FlRefShape<32>::d;
    if (std::memcmp(&s, &cs, sizeof(s)) != 0) fail("run-time row != compile-time row", 0, s.P, cs.P);
    if (!fl_slab_blk_gapfree(d, s)) fail("row has gaps", 0, 0, 1);
    if (s.Pz < s.P || s.Pz - s.P >= 8 || (s.Pz & 7) != 0) fail("zero-filled tail", 0, s.Pz, s.P);
    // kind[pos]: 0 unassigned, 1 weight, 2 pad column, 3 bias -- from the definition
    std::vector<int> kind(s.Pz, 0), want(s.Pz, -1), hits(s.Pz, 0), stores(s.Pz, 0);
    int di = 0, pads = 0;
    for (int l = 0; l < d.L; ++l) {
        const int K = d.dim[l], N = d.dim[l + 1], itiles = (K + 15) / 16, otiles = (N + 15) / 16;
        for (int it = 0; it < itiles; ++it) {
            int w = K - 16 * it < 16 ? K - 16 * it : 16;
            w = (w + 3) / 4 * 4;
            const int off = fl_slab_blk_off(s, l, it);
            if (w != fl_slab_blk_w(K, it)) fail("block width", it, w, fl_slab_blk_w(K, it));
            if (off % 32 != 0) fail("block offset not 64-byte aligned", off, off % 32, 0);
            for (int o = 0; o < N; ++o)
                for (int c = 0; c < w; ++c) {
                    const int pos = off + o * w + c, i = 16 * it + c;
                    if (pos < 0 || pos >= s.P) { fail("block position out of the row", pos, pos, s.P); continue; }
                    if (kind[pos] != 0) fail("position in two blocks", pos, kind[pos], 0);
                    kind[pos] = i < K ? 1 : 2;
                    pads += i >= K;
                    if (i < K) want[pos] = d.w_off[l] + o * K + i;
                }
            // the train kernel's stores (fl_kernels_bf16.hip wgrad_layer_bf16): lane (lr, lg) of tile (ot, it)
            // writes 4 halves at off + o w + 4 lg for o = 16 ot + lr, when o < N and 4 lg < w
            for (int ot = 0; ot < otiles; ++ot)
                for (int lane = 0; lane < 64; ++lane) {
                    const int lr = lane & 15, lg = lane >> 4, o = 16 * ot + lr;
                    if (!(o < N && 4 * lg < w)) continue;
                    const int pos = off + o * w + 4 * lg;
                    if (pos % 4 != 0) fail("store not 8-byte aligned", pos, pos % 4, 0);
                    if (pos < off || pos + 4 > off + N * w) { fail("store outside its block", pos, off, off + N * w); continue; }
                    for (int j = 0; j < 4; ++j) ++stores[pos + j];
                }
        }
        for (int o = 0; o < N; ++o) {
            const int pos = s.b_off[l] + o;
            if (pos < 0 || pos >= s.P) { fail("bias position out of the row", pos, pos, s.P); continue; }
            if (kind[pos] != 0) fail("bias on a block position", pos, kind[pos], 0);
            kind[pos] = 3;
            want[pos] = d.b_off[l] + o;
            ++stores[pos];
        }
        di += N * K + N;
    }
    if (di != d.P) fail("dense indices walked", 0, di, d.P);
    for (int pos = 0; pos < s.P; ++pos) {
        if (kind[pos] == 0) fail("position neither gradient nor pad", pos, 0, 1);
        if (stores[pos] != 1) fail("position not stored exactly once per launch", pos, stores[pos], 1);
        // the inverse map, compile-time and run-time descriptors
        const int a = fl_slab_blk_dense(cd, cs, pos), b = fl_slab_blk_dense(d, s, pos);
        if (a != b) fail("inverse map, static vs run-time", pos, a, b);
        if (a != want[pos]) fail("inverse map", pos, a, want[pos]);
        if ((a < 0) != (kind[pos] == 2)) fail("pads are exactly the i >= K columns", pos, a, kind[pos]);
    }
    for (int pos = s.P; pos < s.Pz + 64; ++pos)
        if (fl_slab_blk_dense(cd, cs, pos) != -1) fail("position past the row maps to a parameter", pos, 0, -1);
    if (fl_slab_blk_dense(cd, cs, -1) != -1) fail("negative position maps to a parameter", -1, 0, -1);
    for (int q = 0; q < d.P; ++q) {
        const int pos = fl_slab_blk_pos(d, s, q);
        if (pos < 0 || pos >= s.P) { fail("forward map out of the row", q, pos, s.P); continue; }
        if (want[pos] != q) fail("forward map", q, want[pos], q);
        if (++hits[pos] != 1) fail("forward map not injective", q, hits[pos], 1);
    }
    int nonpad = 0;
    for (int pos = 0; pos < s.P; ++pos) {
        nonpad += kind[pos] != 2;
        if ((kind[pos] != 2) != (hits[pos] == 1)) fail("non-pad positions are hit exactly once", pos, hits[pos], kind[pos]);
    }
    if (nonpad != d.P) fail("non-pad positions", 0, nonpad, d.P);
    std::printf("indices: %d\nrow halves: %d\npads: %d\nrow floats: %d\nfailures: %d\n", d.P, s.P, pads,
                ((s.P + 1) + 3) & ~3, failures);
    return failures != 0;
}
