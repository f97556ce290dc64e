// Dense parameter index -> where the Adam kernel keeps that parameter: its position in the fp32
// parameter image (fl_common.h) and, bf16 mode, its byte position in the packed LDS-layout image
// relative to the parameter region (MLPDescB::param_off).  One function for every Adam kernel
// (fl_adam_body.inc) and for the host (tests/native/test_adam_map.cpp).
#pragma once
#include "fl_common.h"

struct FlAdamPos {
    int j;         // image index (floats)
    int pk;        // packed byte position: bf16 hi part of a weight, fp32 slot of a bias
    bool is_bias;
};

// kStatic = false (run-time descriptors): the layer's offsets are gathered by compile-time-indexed
// selects -- a per-lane index into the descriptors would read them from memory, a dependent round
// trip in front of the wave's slab loads -- then one division by the gathered fan-in.
// kStatic = true (descriptors that fold, fl_layout.h FlShapeRef): one arm per layer, so every
// division is by that layer's constant fan-in (14, 50, 200 for the reference MLP) and every offset
// an immediate.  Same arithmetic, same result for every index below d.P.
template <bool kStatic>
__host__ __device__ constexpr FlAdamPos fl_adam_pos(const MLPDesc& d, const MLPDescB& e, int di) {
    FlAdamPos r = {0, 0, false};
    if (kStatic) {
#pragma unroll
        for (int t = 0; t < FL_MAX_LAYERS; ++t) {
            if (t >= d.L || di < d.w_off[t] || (t + 1 < d.L && di >= d.w_off[t + 1])) continue;
            if (di < d.b_off[t]) {
                const int K = d.dim[t], q = di - d.w_off[t];
                const int n = q / K, k = q - n * K;
                r.j = d.iw_off[t] + n * fl_ldw(K) + (k ^ fl_swz(n));
                r.pk = e.w_off[t] - e.param_off + fl_wrow(n, e.ldw[t], e.wgap) +
                       ((((k >> 3) ^ fl_wswz(n, e.wxor)) << 4) | ((k & 7) << 1));
            } else {
                r.j = d.ib_off[t] + (di - d.b_off[t]);
                r.pk = e.bias_off[t] - e.param_off + (di - d.b_off[t]) * 4;
                r.is_bias = true;
            }
        }
        return r;
    }
    int K = d.dim[0], wo = d.w_off[0], bo = d.b_off[0], iwo = d.iw_off[0], ibo = d.ib_off[0];
    int ewo = e.w_off[0], ebo = e.bias_off[0], eldw = e.ldw[0];
#pragma unroll
    for (int t = 1; t < FL_MAX_LAYERS; ++t)
        if (t < d.L && di >= d.w_off[t]) {
            K = d.dim[t]; wo = d.w_off[t]; bo = d.b_off[t]; iwo = d.iw_off[t]; ibo = d.ib_off[t];
            ewo = e.w_off[t]; ebo = e.bias_off[t]; eldw = e.ldw[t];
        }
    if (di < bo) {
        const int q = di - wo;
        const int n = q / K, k = q - n * K;
        r.j = iwo + n * fl_ldw(K) + (k ^ fl_swz(n));  // (swizzled image, fl_common.h)
        r.pk = ewo - e.param_off + fl_wrow(n, eldw, e.wgap) + ((((k >> 3) ^ fl_wswz(n, e.wxor)) << 4) | ((k & 7) << 1));
    } else {
        r.j = ibo + (di - bo);
        r.pk = ebo - e.param_off + (di - bo) * 4;
        r.is_bias = true;
    }
    return r;
}
