// The reference shape's compile-time layouts (fl_layout.h FlRefShape) against the run-time layout
// code: for dims {14, 50, 200, 2} at every R with shape-specialised kernels the engine's run-time
// descriptors are byte-equal to the constants, so the launchers' byte comparison picks the
// specialised kernels; for the near-miss shapes they are not.  Stand-alone host program (built
// with AddressSanitizer + UBSan by tests/test_native_layout_constexpr.py).
#include <cstdio>
#include <cstring>

#include "fl_layout.h"

// the layouts are constants of the language, not only equal at run time
static_assert(FlRefShape<32>::d.L == 3 && FlRefShape<32>::d.dim[0] == 14 && FlRefShape<32>::d.dim[3] == 2, "dims");
static_assert(FlRefShape<32>::d.P == 14 * 50 + 50 + 50 * 200 + 200 + 200 * 2 + 2, "dense parameter count");
static_assert(FlRefShape<32>::e.kp[1] == 64 && FlRefShape<32>::e.kp[2] == 224, "padded fan-ins");
static_assert(FlRefShape<32>::e.lds_bytes <= (int)FL_LDS_DYNAMIC_MAX, "train layout fits the LDS");
static_assert(FlRefShape<32>::ev.lds_bytes <= (int)FL_LDS_DYNAMIC_MAX, "evaluation layout fits the LDS");
static_assert(FlRefShape<32>::e.head_split == FlRefShape<32>::ev.head_split, "one logits split");

static int failures = 0;

static void build(const int* dims, int R, MLPDesc* d, MLPDescB* e, MLPDescB* ev) {
    fl_build_fp32_layout(dims, 3, R, d);
    fl_build_bf16_layout(*d, R, e, ev);
}

template <int R>
static void check_r() {
    const int ref[4] = {14, 50, 200, 2};
    MLPDesc d;
    MLPDescB e, ev;
    build(ref, R, &d, &e, &ev);
    const MLPDesc cd = FlRefShape<R>::d;
    const MLPDescB ce = FlRefShape<R>::e, cev = FlRefShape<R>::ev;
    if (std::memcmp(&d, &cd, sizeof(d)) != 0) { std::printf("R=%d: MLPDesc differs\n", R); ++failures; }
    if (std::memcmp(&e, &ce, sizeof(e)) != 0) { std::printf("R=%d: train MLPDescB differs\n", R); ++failures; }
    if (std::memcmp(&ev, &cev, sizeof(ev)) != 0) { std::printf("R=%d: eval MLPDescB differs\n", R); ++failures; }
    if (!fl_ref_shape_match<R>(d, e)) { std::printf("R=%d: reference shape not matched\n", R); ++failures; }
    const int miss[4][4] = {{14, 50, 200, 3}, {15, 50, 200, 2}, {14, 50, 208, 2}, {14, 48, 200, 2}};
    for (const auto& m : miss) {
        build(m, R, &d, &e, &ev);
        if (fl_ref_shape_match<R>(d, e)) {
            std::printf("R=%d: near miss {%d, %d, %d, %d} matched\n", R, m[0], m[1], m[2], m[3]);
            ++failures;
        }
    }
    // a reference shape at another R is no match either (the layout depends on R)
    build(ref, R == 32 ? 16 : 32, &d, &e, &ev);
    if (fl_ref_shape_match<R>(d, e)) { std::printf("R=%d: layout of another R matched\n", R); ++failures; }
    std::printf("R=%d: level %d, %d LDS bytes, head_split %d\n", R, ce.level, ce.lds_bytes, ce.head_split);
}

int main() {
    check_r<32>();  // every R with a specialised kernel (fl_launch_train_bf16, fl_launch_train)
    std::printf("failures: %d\n", failures);
    return failures != 0;
}
