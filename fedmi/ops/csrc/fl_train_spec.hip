// Shape-specialised fp32 train kernel for the reference 14-50-200-2 MLP: the fp32 twin of
// fl_train_bf16_spec.hip, in a translation unit of its own so the generic kernels' code generation
// is untouched.  The body and the device functions are the generic kernel's (fl_train_body.inc,
// fl_kernels.hip) under the static shape policy FlShapeRef<R> (fl_layout.h): no MLPDesc kernel
// argument, every layer's shape, stride and offset a constant, the layer and chunk loops unrolled.
// Same MFMAs in the same order: results are bitwise the generic kernel's (tests/test_shape_spec.py).
// fl_launch_train picks it only for a run-time descriptor byte-equal to the compile-time one.
#define FL_FP32_DEVICE_ONLY
#include "fl_kernels.hip"

template <int RT>
__global__ void __launch_bounds__(FL_THREADS)
fl_train_spec_kernel(FLConfig c, FLBuffers b, const float* __restrict__ pg, const FLState* __restrict__ st_in,
                     FLState* __restrict__ st_out, int local_step, int mode, float* __restrict__ cm_out,
                     int fold_mask) {
    using SP = FlShapeRef<RT * 16>;
    constexpr MLPDesc d = FlRefShape<RT * 16>::d;  // (a local copy: folded, fl_layout.h FL_SHAPE_D)
#include "fl_train_body.inc"
}

bool fl_train_spec_ok(const MLPDesc& d, const FLConfig& c, int mode) {
    const MLPDesc rd = FlRefShape<32>::d;
    return c.R == 32 && mode != FL_EVAL_LAGGED && std::memcmp(&d, &rd, sizeof(d)) == 0;
}

hipError_t fl_launch_train_spec(const FLConfig& c, const FLBuffers& b, const float* pg, const FLState* si, FLState* so,
                                int ls, hipStream_t s, int mode, float* cm_out, int fold_mask) {
    if (c.R != 32 || mode == FL_EVAL_LAGGED || (mode == FL_EVAL_FUSED && cm_out == nullptr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fl_train_spec_kernel<2>, dim3(c.n_slabs), dim3(FL_THREADS),
                       (size_t)FlRefShape<32>::d.lds_floats * sizeof(float), s, c, b, pg, si, so, ls, mode, cm_out,
                       fold_mask);
    return hipGetLastError();
}

hipError_t fl_set_lds_limit_spec(size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(fl_train_spec_kernel<2>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
