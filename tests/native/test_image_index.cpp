// Dense index -> image position of the kernels that run after the Adam kernel (fl_image.h
// fl_image_index) on the host, for every dense index of a sweep of shapes: it is the Adam kernels' map
// (fl_adam_map.h, run-time arm), it stays inside the image, hits no slot twice, lands on a float that
// fl_image_lim calls a real parameter, and fl_image_lim calls exactly P floats real -- so the map is onto
// the real set and the rule and its inverse agree.
// Stand-alone host program (built with AddressSanitizer + UBSan by tests/test_native_image_index.py).
#include <cstdio>
#include <vector>

#include "fl_adam_map.h"
#include "fl_image.h"
#include "fl_layout.h"

// usable in constant expressions: the last bias of the reference shape
static_assert(fl_image_index(FlRefShape<32>::d, FlRefShape<32>::d.P - 1) == FlRefShape<32>::d.ib_off[2] + 1, "last bias");

static int failures = 0;
static void fail(const char* what, int shape, int di, int a, int b) {
    if (++failures <= 20) std::printf("shape %d index %d: %s %d vs %d\n", shape, di, what, a, b);
}

int main() {
    const int shapes[7][FL_MAX_LAYERS + 2] = {  // {L, dims...}
        {3, 14, 50, 200, 2}, {2, 17, 24, 3}, {2, 1, 16, 2}, {2, 33, 65, 3}, {4, 14, 33, 17, 9, 5}, {1, 14, 7},
        {3, 40, 40, 96, 4}};
    int indices = 0;
    for (int s = 0; s < 7; ++s) {
        const int L = shapes[s][0];
        MLPDesc d;
        MLPDescB e, ev;
        fl_build_fp32_layout(shapes[s] + 1, L, 32, &d);
        fl_build_bf16_layout(d, 32, &e, &ev);
        std::vector<int> hits(d.Pimg, 0);
        for (int di = 0; di < d.P; ++di, ++indices) {
            const int j = fl_image_index(d, di);
            const int a = fl_adam_pos<false>(d, e, di).j;
            if (j != a) fail("fl_image_index vs fl_adam_pos", s, di, j, a);
            if (j < 0 || j >= d.Pimg) { fail("outside the image", s, di, j, d.Pimg); continue; }
            if (++hits[j] > 1) fail("image slot hit twice", s, di, j, hits[j]);
            const int lim = fl_image_lim(d, j & ~3);
            if (!((j & 3) < lim)) fail("not a real parameter by fl_image_lim", s, di, j & 3, lim);
        }
        int real = 0;
        for (int q = 0; q < d.Pimg; q += 4) {
            const int lim = fl_image_lim(d, q);
            real += lim < 0 ? 0 : (lim > 4 ? 4 : lim);
        }
        if (real != d.P) fail("floats fl_image_lim calls real vs P", s, -1, real, d.P);
    }
    std::printf("indices: %d\nfailures: %d\n", indices, failures);
    return failures != 0;
}
