// Update compression with error feedback (a SIMULATION of a compressed uplink: the exchange still
// carries the dense fp32 image, only the information in it changes): one launch per round, after
// the last local step's Adam kernel, rewrites the parameter image of the round's FedAvg
// contribution in the comm buffer.  With x the image the round trained from, e the client's
// residual (0 at start), the FedAvg weight w (rtab), on the P real parameters, every operation an
// fp32 round-to-nearest one:
//
//   u  = (local - x) + e
//   c  = C(u)           top-k : the k entries of largest |u| keep c = u, the rest c = 0
//                       sign  : c = copysign(s, u), s = (sum |u|) / P
//   e' = error_feedback ? (kept ? 0 : u - c) : 0       (sign keeps nothing)
//   contribution = w * (x + c)                          image padding stays exact 0
//
// A round that is not live is left untouched; a client that is not sampled (w = 0) keeps its
// contribution (the Adam kernel's zeros) and carries its residual over unchanged.
//
// The residual is double-buffered by round parity (round r reads half r & 1 and writes half
// (r + 1) & 1 of FLCompress::residual): every workgroup needs the WHOLE old residual for the
// threshold, and there is no grid barrier that would keep a fast workgroup's new entries out of a
// slow workgroup's reads.
//
// Every workgroup recomputes the whole selection itself (both images and the residual come from
// L2) and keeps the P values of u in LDS:
//   top-k : a radix select over the 31-bit magnitude keys (bits & 0x7fffffff, so any NaN ranks
//           above inf), 8 + 8 + 8 + 7 bits, largest first, gives the k-th largest key T and how many
//           entries equal to T are kept; the same select over the 16-bit dense indices of the entries
//           equal to T, smallest first, gives the index cut-off among the ties.  Integer LDS
//           histogram counts only: their result does not depend on the order of the adds.
//   sign  : sum |u| in ONE fixed order -- per thread the dense entries t, t + 1024, ..., an xor tree
//           over the wave, the 16 waves' sums in wave order -- so all workgroups hold a bit-identical
//           s and a run is bitwise repeatable.
// Every loop has a trip count fixed by the launch (ceil(P / 1024) entries per thread, taken four at a
// time; 6 passes).
// fedmi/fl/compress.py is the host model.
#include "fl_common.h"
#include "fl_device.h"
#include "fl_image.h"

#define FL_CP_THREADS 1024
#define FL_CP_BINS 256

// One pass of a radix select.  `hist` holds the counts of the pass's digit over the entries still in
// play; `want` (1 <= want <= their number) is the rank looked for, counted from the highest digit.
// Wave 0 finds the digit holding that rank and the rank within it: lane l owns bins 4l .. 4l + 3,
// a suffix scan over the lanes gives the count above each bin.  sel[0] = digit, sel[1] = rank in it.
__device__ __forceinline__ void cp_pick(const int* hist, int want, int* sel) {
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 64) {
        const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
        const int tot = h0 + h1 + h2 + h3;
        int v = tot;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_down(v, off, 64);
            if (lane + off < 64) v += t;
        }
        int above = v - tot;  // entries in the bins of higher lanes
        const int hb[4] = {h3, h2, h1, h0};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (above < want && above + hb[b] >= want) {
                sel[0] = 4 * lane + 3 - b;
                sel[1] = want - above;
            }
            above += hb[b];
        }
    }
}

__global__ void __launch_bounds__(FL_CP_THREADS)
fl_compress_kernel(MLPDesc d, FLCompress p, const float* __restrict__ local, const float* __restrict__ pg,
                   float* __restrict__ comm, const FLState* __restrict__ st, const float* __restrict__ rtab) {
    extern __shared__ float ubuf[];  // [P] u of every real parameter, dense order
    __shared__ int hist[FL_CP_BINS];
    __shared__ int sel[2];
    __shared__ float wsum[FL_CP_THREADS / 64];
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;  // past a stop / max_rounds: the Adam kernel republished the global image
    const float w = fl_round_weight(rtab, r);
    const float* __restrict__ ein = p.residual + (size_t)(r & 1) * d.Pimg;
    float* __restrict__ eout = p.residual + (size_t)((r + 1) & 1) * d.Pimg;
    const int q = blockIdx.x * FL_CP_THREADS + threadIdx.x;  // block of 4 dense parameters
    if (w == 0.f) {  // not sampled this round: zeros from the Adam kernel; the residual carries over
        if (blockIdx.x == 0 && threadIdx.x == 0) p.stat_hist[r] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int di = 4 * q + k;
            if (di < d.P) {
                const int j = fl_image_index(d, di);
                eout[j] = ein[j];
            }
        }
        return;
    }
    const int P = d.P;
    const int per = (P + FL_CP_THREADS - 1) / FL_CP_THREADS;  // entries per thread: t, t + 1024, ...

    // Entries are taken four at a time with unconditional loads (index clamped into the model), so a
    // thread has 12 global / 4 LDS loads in flight instead of waiting for each entry's in turn: one
    // 1024-thread workgroup per CU has little else to hide the latency with.
    float acc = 0.f;
    for (int it = 0; it < per; it += 4) {
        float a[4], x[4], e[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int di = (it + i) * FL_CP_THREADS + threadIdx.x;
            const int j = fl_image_index(d, di < P ? di : P - 1);
            a[i] = local[j]; x[i] = pg[j]; e[i] = ein[j];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int di = (it + i) * FL_CP_THREADS + threadIdx.x;
            if (di < P) {
                const float u = __fadd_rn(__fsub_rn(a[i], x[i]), e[i]);
                ubuf[di] = u;
                acc = __fadd_rn(acc, fabsf(u));
            }
        }
    }

    float s = 0.f;          // sign: the scale; top-k: unused
    unsigned thr = 0;       // top-k: key of the k-th largest magnitude
    int cut = 0;            // top-k: entries with that key are kept up to this dense index
    if (p.kind == FL_COMPRESS_SIGN) {
        s = __fdiv_rn(block_sum_ordered<FL_CP_THREADS>(acc, wsum), (float)P);
        if (blockIdx.x == 0 && threadIdx.x == 0) p.stat_hist[r] = s;
    } else {
        int want = p.k;
        // magnitude keys, largest first: digits of 8, 8, 8 and 7 bits below the sign bit
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = pass < 3 ? 23 - 8 * pass : 0;
            const int bits = pass < 3 ? 8 : 7;
            if (threadIdx.x < FL_CP_BINS) hist[threadIdx.x] = 0;
            __syncthreads();  // (first pass: also orders the ubuf stores before the reads)
            // a thread's consecutive entries with one digit (the exponent pass: most of them) make one add
            int run_d = -1, run_n = 0;
            for (int it = 0; it < per; it += 4) {
                unsigned key[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int di = (it + i) * FL_CP_THREADS + threadIdx.x;
                    key[i] = __float_as_uint(ubuf[di < P ? di : P - 1]) & 0x7fffffffu;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int di = (it + i) * FL_CP_THREADS + threadIdx.x;
                    if (di < P && (key[i] >> (shift + bits)) == (thr >> (shift + bits))) {  // (first pass: 0 == 0)
                        const int dg = (int)((key[i] >> shift) & ((1u << bits) - 1u));
                        if (dg != run_d) {
                            if (run_n) atomicAdd(&hist[run_d], run_n);
                            run_d = dg;
                            run_n = 0;
                        }
                        ++run_n;
                    }
                }
            }
            if (run_n) atomicAdd(&hist[run_d], run_n);
            __syncthreads();
            cp_pick(hist, want, sel);
            __syncthreads();
            thr |= (unsigned)sel[0] << shift;
            want = sel[1];
        }
        // dense indices of the entries equal to the threshold, smallest first: 2 digits of 8 bits
        // (the select above counts from the highest digit, so the digit is complemented)
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int shift = 8 - 8 * pass;
            if (threadIdx.x < FL_CP_BINS) hist[threadIdx.x] = 0;
            __syncthreads();
            for (int it = 0; it < per; it += 4) {
                unsigned key[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int di = (it + i) * FL_CP_THREADS + threadIdx.x;
                    key[i] = __float_as_uint(ubuf[di < P ? di : P - 1]) & 0x7fffffffu;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int di = (it + i) * FL_CP_THREADS + threadIdx.x;
                    if (di < P && key[i] == thr && (pass == 0 || (di >> 8) == (cut >> 8)))
                        atomicAdd(&hist[255 - ((di >> shift) & 255)], 1);
                }
            }
            __syncthreads();
            cp_pick(hist, want, sel);
            __syncthreads();
            cut |= (255 - sel[0]) << shift;
            want = sel[1];
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) p.stat_hist[r] = __uint_as_float(thr);
    }

#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int di = 4 * q + k;
        if (di >= P) break;
        const int j = fl_image_index(d, di);
        const float u = ubuf[di];
        float c, en;
        if (p.kind == FL_COMPRESS_SIGN) {
            c = copysignf(s, u);
            en = __fsub_rn(u, c);
        } else {
            const unsigned key = __float_as_uint(u) & 0x7fffffffu;
            const bool kept = key > thr || (key == thr && di <= cut);
            c = kept ? u : 0.f;
            en = kept ? 0.f : u;
        }
        comm[j] = __fmul_rn(w, __fadd_rn(pg[j], c));
        eout[j] = p.error_feedback ? en : 0.f;
    }
}

// Dynamic LDS of the kernel for this model (P floats); call once before the first launch (the engine's
// constructor does), not inside a stream capture.
hipError_t fl_set_lds_limit_compress(const MLPDesc& d) {
    const size_t lds = (size_t)d.P * sizeof(float);
    if (d.P < 1 || lds > (size_t)FL_LDS_DYNAMIC_MAX) return hipErrorInvalidValue;  // (fits no fused kernel either)
    return hipFuncSetAttribute(reinterpret_cast<const void*>(fl_compress_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

hipError_t fl_launch_compress(const MLPDesc& d, const FLCompress& p, const float* local, const float* pg, float* comm,
                              const FLState* st, const float* rtab, hipStream_t s) {
    if ((d.Pimg & 3) != 0 || d.P < 1 || d.P > 65536 || (size_t)d.P * sizeof(float) > (size_t)FL_LDS_DYNAMIC_MAX ||
        (p.kind != FL_COMPRESS_TOPK && p.kind != FL_COMPRESS_SIGN) || p.P != d.P || p.k < 1 || p.k > d.P ||
        p.residual == nullptr || p.stat_hist == nullptr || p.max_rounds < 1)
        return hipErrorInvalidValue;
    const int quads = (d.P + 3) / 4;
    hipLaunchKernelGGL(fl_compress_kernel, dim3((quads + FL_CP_THREADS - 1) / FL_CP_THREADS), dim3(FL_CP_THREADS),
                       (size_t)d.P * sizeof(float), s, d, p, local, pg, comm, st, rtab);
    return hipGetLastError();
}
