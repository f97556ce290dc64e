// Shape-specialised bf16 train kernel for the reference 14-50-200-2 MLP, in a translation unit of
// its own so the generic kernels' code generation is untouched (as fl_adam_local.hip).  The body and
// the device functions are the generic kernel's (fl_train_bf16_body.inc, fl_kernels_bf16.hip) under
// the static shape policy FlShapeRef<R> (fl_layout.h): the model shape and the LDS layout are the
// compiler-evaluated constants of FlRefShape<R> instead of the MLPDesc / MLPDescB kernel arguments
// (384 bytes less per launch, no descriptor loads between the phases), and the layer, K and tile
// loops are unrolled with constant trip counts and immediate LDS offsets.  Same MFMAs in the same
// order into the same accumulators, same epilogues and slab stores: results are bitwise the generic
// kernel's (tests/test_shape_spec.py).  fl_launch_train_bf16 picks it only for run-time
// descriptors that are byte-equal to the constants.
// The blocked instantiation (BLK) writes the fp16 slab row in the blocked order of fl_layout.h
// (FlSlabBlk): the weight-gradient MFMA's operands exchange roles, so a lane holds 4 consecutive inputs
// of one output and a 16 x 16 tile leaves as one 8-byte store per lane, a contiguous 64-byte-aligned run
// of at most 512 bytes, instead of four 2-byte stores per lane in 32-byte pieces 2 K bytes apart.  Same
// accumulator bits, same rounding and store policy; only the place in the row differs
// (tests/test_slab_blocked.py; profiles/slab_blocked_probe.log, profiles/slab_blocked_ab.log).
#define FL_BF16_DEVICE_ONLY
#include "fl_kernels_bf16.hip"

// BLK: the fp16 slab row is the blocked one (fl_layout.h FlSlabBlk; read back by the blocked
// instantiation of fl_adam_spec.hip alone); false: the dense row every Adam kernel reads.
// EPI: the hidden layers' forward tiles and the dgrad tiles are computed transposed (exchanged MFMA
// operands, fl_layout.h fl_epi_*), so a lane holds 4 consecutive columns of one row and its bf16 results
// leave as one 8-byte LDS store instead of four 2-byte ones, rounded two per v_cvt_pk_bf16_f32.  Same
// accumulator bits, same LDS bytes (tests/test_epilogue_exchange.py); false: the generic epilogues.
template <int RT, int LAG, bool PLAIN, bool BLK, bool EPI>
__global__ void __launch_bounds__(FL_THREADS)
fl_train_bf16_spec_kernel(FLConfig c, FLBuffers b, const float* __restrict__ pg, const FLState* __restrict__ st_in,
                          FLState* __restrict__ st_out, int local_step, int stage_local, int mode,
                          float* __restrict__ cm_out, int fold_mask) {
    using SP = FlShapeRef<RT * 16, BLK, EPI>;
    constexpr MLPDesc d = FlRefShape<RT * 16>::d;  // (local copies: folded, fl_layout.h FL_SHAPE_D)
    constexpr MLPDescB e = FlRefShape<RT * 16>::e;
#include "fl_train_bf16_body.inc"
}

// One client, R = 32, split-bf16 forward, no lagged scoring: the round bench.py's headline times.
bool fl_train_bf16_spec_ok(const MLPDesc& d, const MLPDescB& e, const FLConfig& c, int mode) {
    return c.R == 32 && mode != FL_EVAL_LAGGED && !c.plain_fwd && fl_ref_shape_match<32>(d, e);
}

template <bool BLK, bool EPI>
static void fl_train_bf16_spec_go(const FLConfig& c, const FLBuffers& b, const float* pg, const FLState* si, FLState* so,
                                  int ls, hipStream_t s, bool stage_local, int mode, float* cm_out, int fold_mask) {
    hipLaunchKernelGGL((fl_train_bf16_spec_kernel<2, 0, false, BLK, EPI>), dim3(c.n_slabs), dim3(FL_THREADS),
                       (size_t)FlRefShape<32>::e.lds_bytes, s, c, b, pg, si, so, ls, stage_local ? 1 : 0, mode, cm_out,
                       fold_mask);
}

hipError_t fl_launch_train_bf16_spec(const FLConfig& c, const FLBuffers& b, const float* pg, const FLState* si,
                                     FLState* so, int ls, hipStream_t s, bool stage_local, int mode, float* cm_out,
                                     int fold_mask, bool slab_blocked, bool epi_exchange) {
    if (c.R != 32 || mode == FL_EVAL_LAGGED || c.plain_fwd) return hipErrorInvalidValue;
    if (mode == FL_EVAL_FUSED && cm_out == nullptr) return hipErrorInvalidValue;
    // the blocked row: fp16 partials, and rows as far apart as its length needs
    if (slab_blocked && (!c.slab_f16 || c.slab_stride < FlRefSlabBlk<32>::s.P + 1)) return hipErrorInvalidValue;
    auto go = slab_blocked ? (epi_exchange ? fl_train_bf16_spec_go<true, true> : fl_train_bf16_spec_go<true, false>)
                           : (epi_exchange ? fl_train_bf16_spec_go<false, true> : fl_train_bf16_spec_go<false, false>);
    go(c, b, pg, si, so, ls, s, stage_local, mode, cm_out, fold_mask);
    return hipGetLastError();
}

hipError_t fl_set_lds_limit_bf16_spec(size_t bytes) {
    const void* fns[4] = {reinterpret_cast<const void*>(fl_train_bf16_spec_kernel<2, 0, false, false, false>),
                          reinterpret_cast<const void*>(fl_train_bf16_spec_kernel<2, 0, false, true, false>),
                          reinterpret_cast<const void*>(fl_train_bf16_spec_kernel<2, 0, false, false, true>),
                          reinterpret_cast<const void*>(fl_train_bf16_spec_kernel<2, 0, false, true, true>)};
    for (const void* fn : fns) {
        const hipError_t err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}
