// The (lane, j) -> (row, column) maps of the exchanged epilogues of the specialised bf16 train kernel
// (fl_layout.h fl_epi_*; fl_kernels_bf16.hip fwd_layer_bf16 / dgrad_layer_bf16 under SP::kEpiExchange), on
// the reference 14-50-200-2 MLP at R = 32: for every tile of both hidden layers' forward pass and every
// dgrad item, each (row, column) of the output buffer's [R][kp] part is produced by exactly one (lane, j),
// every lane's 4 columns are consecutive, its 8-byte store (and the 8-byte mask read of dgrad, the 16-byte
// bias read of the forward pass) is aligned and inside its buffer's extent from FlRefShape<32>::e, and the
// forward column is the W row the lane's operand was loaded from (fl_fwd_col).
// Stand-alone host program (built with AddressSanitizer + UBSan by tests/test_native_epi_map.py).
#include <cstdio>
#include <vector>

#include "fl_layout.h"

static_assert(fl_epi_fwd_col(0, 0, 0) == 4 && fl_epi_fwd_col(0, 48, 0) == 0, "lane group g: columns 4 ((g + 1) & 3)..");
static_assert(fl_epi_dgrad_col(1, 17, 3) == 16 + 4 + 3 && fl_epi_row(1, 17) == 17, "dgrad: features 4 g.. of row lr");

static int failures = 0;
static void fail(const char* what, int at, int a, int b) {
    if (++failures <= 20) std::printf("%d: %s %d != %d\n", at, what, a, b);
}

// One epilogue: `tiles` column tiles of 16 over RT row tiles into the bf16 buffers at byte offsets offs[0..nb)
// of row stride lda elements; fwd: the forward map (else dgrad's).
static int walk(const MLPDescB& e, int R, int tiles, int lda, const int* offs, int nb, bool fwd, int bias_off, int kp) {
    const int RT = R / 16;
    std::vector<int> hits((size_t)R * kp, 0);
    int stores = 0;
    for (int t = 0; t < tiles; ++t)
        for (int rt = 0; rt < RT; ++rt)
            for (int lane = 0; lane < 64; ++lane) {
                const int row = fl_epi_row(rt, lane);
                const int c0 = fwd ? fl_epi_fwd_col(t, lane, 0) : fl_epi_dgrad_col(t, lane, 0);
                for (int j = 0; j < 4; ++j) {
                    const int col = fwd ? fl_epi_fwd_col(t, lane, j) : fl_epi_dgrad_col(t, lane, j);
                    if (col != c0 + j) fail("columns of a lane not consecutive", lane, col, c0 + j);
                    // accumulator 4 lg + j of the transposed tile: the output of the operand row lane 4 lg + j loaded
                    const int m = 4 * (lane >> 4) + j;
                    const int want = t * 16 + (fwd ? fl_fwd_col(m) : m);
                    if (col != want) fail("column is not the operand row's", lane, col, want);
                    if (row < 0 || row >= R || col < 0 || col >= kp) { fail("element outside [R][kp]", lane, row, col); continue; }
                    ++hits[(size_t)row * kp + col];
                }
                if (row != rt * 16 + (lane & 15)) fail("row", lane, row, rt * 16 + (lane & 15));
                const int o = fl_epi_off(row, c0, lda);
                if (o % 8 != 0) fail("store not 8-byte aligned", lane, o % 8, 0);
                if (o < 0 || o + 8 > R * lda * 2) fail("store outside its buffer", lane, o, R * lda * 2);
                for (int q = 0; q < nb; ++q) {
                    if ((offs[q] + o) % 8 != 0) fail("LDS address not 8-byte aligned", lane, (offs[q] + o) % 8, 0);
                    if (offs[q] < 0 || offs[q] + o + 8 > e.lds_bytes) fail("store outside the LDS layout", lane, offs[q] + o, e.lds_bytes);
                }
                if (fwd) {  // 16-byte read of 4 fp32 biases
                    const int bo = bias_off + c0 * 4;
                    if (bo % 16 != 0) fail("bias read not 16-byte aligned", lane, bo % 16, 0);
                    if (c0 + 4 > kp) fail("bias read past the padded biases", lane, c0 + 4, kp);
                }
                ++stores;
            }
    for (int r = 0; r < R; ++r)
        for (int c = 0; c < kp; ++c)
            if (hits[(size_t)r * kp + c] != 1) fail("element not produced exactly once", r * kp + c, hits[(size_t)r * kp + c], 1);
    return stores;
}

int main() {
    constexpr int R = 32;
    const MLPDesc d = FlRefShape<R>::d;
    const MLPDescB e = FlRefShape<R>::e;
    int stores = 0, elems = 0;
    // buffers of one [R][lda] shape must not run into each other: extents from the layout's own offsets
    for (int l = 1; l < d.L; ++l) {
        const int bytes = R * e.lda[l] * 2;
        const int offs[3] = {e.act_off[l], e.alo_off[l], e.dlt_off[l]};
        for (int q = 0; q < 3; ++q) {
            if (offs[q] % 16 != 0) fail("buffer not 16-byte aligned", l, offs[q] % 16, 0);
            if (offs[q] + bytes > e.param_off) fail("buffer runs into the parameter region", l, offs[q] + bytes, e.param_off);
        }
        if (e.alo_off[l] != e.dlt_off[l]) fail("hidden lo parts live in the delta buffers", l, e.alo_off[l], e.dlt_off[l]);
        if (e.act_off[l] + bytes > e.act_off[l + 1] && l + 1 < d.L) fail("act buffers overlap", l, e.act_off[l] + bytes, e.act_off[l + 1]);
    }
    // forward of the hidden layers l = 0 .. L-2: tiles of kp[l+1] columns into act_{l+1} and alo_{l+1}
    for (int l = 0; l + 1 < d.L; ++l) {
        const int offs[2] = {e.act_off[l + 1], e.alo_off[l + 1]};
        if (e.bias_off[l] % 16 != 0) fail("bias block not 16-byte aligned", l, e.bias_off[l] % 16, 0);
        stores += walk(e, R, e.kp[l + 1] >> 4, e.lda[l + 1], offs, 2, true, e.bias_off[l], e.kp[l + 1]);
        elems += R * e.kp[l + 1];
    }
    // dgrad of layers l = L-1 .. 1: items of kp[l] features into D_l, masked by act_l
    for (int l = d.L - 1; l >= 1; --l) {
        const int offs[2] = {e.dlt_off[l], e.act_off[l]};
        stores += walk(e, R, e.kp[l] >> 4, e.lda[l], offs, 2, false, 0, e.kp[l]);
        elems += R * e.kp[l];
    }
    std::printf("lane stores: %d\nelements: %d\nfailures: %d\n", stores, elems, failures);
    return failures != 0;
}
