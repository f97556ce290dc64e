// The Adam kernels' map from dense parameter index to image index / packed byte position / bias flag
// (fl_adam_map.h): the arm the specialised kernel compiles -- one branch per layer, evaluated with the
// FlRefShape<32> constants -- against the generic arm on the engine's run-time descriptors, for every
// dense index of the reference 14-50-200-2 MLP; and both against the definition of the two layouts
// (fl_common.h: swizzled fp32 image, packed bf16 image), with every real parameter hit exactly once.
// Stand-alone host program (built with AddressSanitizer + UBSan by tests/test_native_adam_map.py).
#include <cstdio>
#include <vector>

#include "fl_adam_map.h"
#include "fl_layout.h"

// the specialised arm is usable in constant expressions with the reference constants
static_assert(fl_adam_pos<true>(FlRefShape<32>::d, FlRefShape<32>::e, 0).j == FlRefShape<32>::d.iw_off[0], "first weight");
static_assert(fl_adam_pos<true>(FlRefShape<32>::d, FlRefShape<32>::e, 14 * 50).is_bias, "first bias");
static_assert(fl_adam_pos<true>(FlRefShape<32>::d, FlRefShape<32>::e, FlRefShape<32>::d.P - 1).j ==
                  FlRefShape<32>::d.ib_off[2] + 1,
              "last bias");

static int failures = 0;
static void fail(const char* what, int di, int a, int b) {
    if (++failures <= 20) std::printf("index %d: %s %d != %d\n", di, what, a, b);
}

int main() {
    const int dims[4] = {14, 50, 200, 2};
    MLPDesc d;
    MLPDescB e, ev;
    fl_build_fp32_layout(dims, 3, 32, &d);
    fl_build_bf16_layout(d, 32, &e, &ev);
    const MLPDesc cd = FlRefShape<32>::d;
    const MLPDescB ce = FlRefShape<32>::e;
    std::vector<int> img_hits(d.Pimg, 0), pk_hits(e.param_bytes, 0);
    int di = 0;
    for (int l = 0; l < d.L; ++l) {
        const int K = d.dim[l], N = d.dim[l + 1];
        for (int q = 0; q < N * K + N; ++q, ++di) {
            const bool bias = q >= N * K;
            const int n = bias ? q - N * K : q / K, k = bias ? 0 : q % K;
            // the definition: fl_common.h image layout and fl_wbyte
            const int j = bias ? d.ib_off[l] + n : d.iw_off[l] + n * fl_ldw(K) + (k ^ fl_swz(n));
            const int pk = bias ? e.bias_off[l] - e.param_off + 4 * n : e.w_off[l] - e.param_off + fl_wbyte(e, l, n, k);
            const FlAdamPos s = fl_adam_pos<true>(cd, ce, di), g = fl_adam_pos<false>(d, e, di);
            if (s.j != g.j) fail("image index, static vs run-time", di, s.j, g.j);
            if (s.pk != g.pk) fail("packed position, static vs run-time", di, s.pk, g.pk);
            if (s.is_bias != g.is_bias) fail("bias flag, static vs run-time", di, s.is_bias, g.is_bias);
            if (s.j != j) fail("image index", di, s.j, j);
            if (s.pk != pk) fail("packed position", di, s.pk, pk);
            if (s.is_bias != bias) fail("bias flag", di, s.is_bias, bias);
            if (s.j < 0 || s.j >= d.Pimg) { fail("image index out of range", di, s.j, d.Pimg); continue; }
            const int bytes = bias ? 4 : 2;  // a weight's lo part lies wlo_delta further, inside the region too
            if (s.pk < 0 || s.pk + (bias ? 0 : e.wlo_delta) + bytes > e.param_bytes) {
                fail("packed position out of range", di, s.pk, e.param_bytes);
                continue;
            }
            ++img_hits[s.j];
            for (int t = 0; t < bytes; ++t) {
                ++pk_hits[s.pk + t];
                if (!bias) ++pk_hits[s.pk + e.wlo_delta + t];
            }
        }
    }
    if (di != d.P) fail("dense indices walked", di, di, d.P);
    for (int j = 0; j < d.Pimg; ++j)
        if (img_hits[j] > 1) fail("image slot written more than once", j, img_hits[j], 1);
    for (int p = 0; p < e.param_bytes; ++p)
        if (pk_hits[p] > 1) fail("packed byte written more than once", p, pk_hits[p], 1);
    std::printf("indices: %d\nfailures: %d\n", di, failures);
    return failures != 0;
}
