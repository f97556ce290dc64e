// fp32 <-> bf16 bit conversions of the split-bf16 parameter images (fl_common.h MLPDescB): shared by
// the bf16 round kernels (fl_kernels_bf16.hip) and the server-optimizer kernel (fl_server.hip),
// whose packed images must agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// fp32 -> bf16 bits, round to nearest even (finite inputs)
__device__ __forceinline__ uint32_t bf16_bits(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) { return bf16_bits(a) | (bf16_bits(b) << 16); }
// lo parts of the split-bf16 representation: bf16(x - bf16(x))
__device__ __forceinline__ uint32_t lo_bits(float x) { return bf16_bits(x - bf16_to_f32((uint16_t)bf16_bits(x))); }
__device__ __forceinline__ uint32_t pack_lo_bf16x2(float a, float b) { return lo_bits(a) | (lo_bits(b) << 16); }
