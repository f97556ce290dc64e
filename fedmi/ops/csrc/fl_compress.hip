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
//
// Two stochastic compressors run in a second entry, fl_compress_random_kernel<kind>, so that the code of
// the two above does not change; they share the loads, the not-sampled path and the select passes with
// it through the functions below.  Dense parameter p takes word p % 4 of Philox4x32-10 at counter
// (p / 4, round, client, stream) under the client's seed: a thread's quad of 4 dense parameters is one
// Philox block, and the round comes from the device state, so a replayed graph draws fresh words.
//   qsgd  : norm = sqrt(sum u * u) in the sign compressor's fixed order (no u array in LDS: the output pass
//           re-reads its quad's three inputs); a = min(|u| / norm * s, s), level = floor(a) + ((word >> 8) <
//           frac(a) * 2^24), c = copysign(norm * level / s, u), e' = u - c.  norm 0 or not finite: c = u, e' = 0.
//   randk : the dynamic LDS array holds key31 = word >> 1 of every parameter instead of u's bits (each
//           thread generates the blocks of quads t, t + 1024, ..., one 16-byte LDS store each), the same
//           six select passes give the k-th largest key and the index cut-off among its ties; the output
//           pass re-reads u from global memory.  With error feedback c = u on kept entries and e' = u
//           elsewhere (the memory variant); without it c = u * (P / k) on kept entries (unbiased), e' = 0.
// All LDS of that entry is dynamic, the select's scratch first, so the key array starts 16-byte aligned.
// fedmi/fl/compress.py is the host model.
#include "fl_common.h"
#include "fl_device.h"
#include "fl_image.h"
#include "fl_philox.h"

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

// A client that is not sampled this round (w = 0): zeros from the Adam kernel stay its contribution; the
// residual of quad q carries over to the half the next round reads.
__device__ __forceinline__ void cp_not_sampled(const MLPDesc& d, const FLCompress& p, int r, int q,
                                               const float* __restrict__ ein, float* __restrict__ eout) {
    if (blockIdx.x == 0 && threadIdx.x == 0) p.stat_hist[r] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int di = 4 * q + k;
        if (di < d.P) {
            const int j = fl_image_index(d, di);
            eout[j] = ein[j];
        }
    }
}

// The three inputs of a thread's entries it .. it + 3 (dense indices (it + i) * 1024 + t), loaded
// unconditionally with the index clamped into the model: 12 global loads in flight per thread.
__device__ __forceinline__ void cp_load4(const MLPDesc& d, int P, int it, const float* __restrict__ local,
                                         const float* __restrict__ pg, const float* __restrict__ ein,
                                         float (&a)[4], float (&x)[4], float (&e)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int di = (it + i) * FL_CP_THREADS + threadIdx.x;
        const int j = fl_image_index(d, di < P ? di : P - 1);
        a[i] = local[j]; x[i] = pg[j]; e[i] = ein[j];
    }
}

// The radix select over the P 31-bit keys in LDS (`keys`: the sign bit is masked off), largest first:
// `thr` = the k-th largest key; the entries equal to it are kept up to dense index `cut` (ties go to the
// lower index).  Ends behind a barrier; `hist` [FL_CP_BINS] and `sel` [2] are LDS scratch.
__device__ __forceinline__ void cp_select(const unsigned* keys, int P, int per, int k, int* hist, int* sel,
                                          unsigned& thr, int& cut) {
    int want = k;
    // keys, largest first: digits of 8, 8, 8 and 7 bits below the sign bit
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = pass < 3 ? 23 - 8 * pass : 0;
        const int bits = pass < 3 ? 8 : 7;
        if (threadIdx.x < FL_CP_BINS) hist[threadIdx.x] = 0;
        __syncthreads();  // (first pass: also orders the key stores before the reads)
        // a thread's consecutive entries with one digit (the exponent pass: most of them) make one add
        int run_d = -1, run_n = 0;
        for (int it = 0; it < per; it += 4) {
            unsigned key[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int di = (it + i) * FL_CP_THREADS + threadIdx.x;
                key[i] = keys[di < P ? di : P - 1] & 0x7fffffffu;
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
                key[i] = keys[di < P ? di : P - 1] & 0x7fffffffu;
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
        cp_not_sampled(d, p, r, q, ein, eout);
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
        cp_load4(d, P, it, local, pg, ein, a, x, e);
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
        // magnitude keys: u's bits below the sign bit
        cp_select(reinterpret_cast<const unsigned*>(ubuf), P, per, p.k, hist, sel, thr, cut);
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

// LDS of the stochastic entry, all dynamic: the select's histogram, its result, the wave sums -- 1104
// bytes, a multiple of 16 -- then (randk) one 31-bit key per parameter, rounded up to whole quads.
#define FL_CP_R_SEL (FL_CP_BINS)
#define FL_CP_R_WSUM (FL_CP_BINS + 4)
#define FL_CP_R_KEYS (FL_CP_BINS + 4 + FL_CP_THREADS / 64)
static inline size_t cp_random_lds(int kind, int P) {
    return sizeof(int) * ((size_t)FL_CP_R_KEYS + (kind == FL_COMPRESS_RANDK ? 4 * (((size_t)P + 3) / 4) : 0));
}

template <int KIND>
__global__ void __launch_bounds__(FL_CP_THREADS)
fl_compress_random_kernel(MLPDesc d, FLCompress p, const float* __restrict__ local, const float* __restrict__ pg,
                          float* __restrict__ comm, const FLState* __restrict__ st, const float* __restrict__ rtab) {
    extern __shared__ __attribute__((aligned(16))) unsigned cp_lds[];
    int* hist = reinterpret_cast<int*>(cp_lds);
    int* sel = reinterpret_cast<int*>(cp_lds) + FL_CP_R_SEL;
    float* wsum = reinterpret_cast<float*>(cp_lds) + FL_CP_R_WSUM;
    unsigned* keys = cp_lds + FL_CP_R_KEYS;  // randk: [4 ceil(P / 4)] key31 of every parameter, dense order
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;
    const float w = fl_round_weight(rtab, r);
    const float* __restrict__ ein = p.residual + (size_t)(r & 1) * d.Pimg;
    float* __restrict__ eout = p.residual + (size_t)((r + 1) & 1) * d.Pimg;
    const int q = blockIdx.x * FL_CP_THREADS + threadIdx.x;  // block of 4 dense parameters = one Philox block
    if (w == 0.f) {
        cp_not_sampled(d, p, r, q, ein, eout);
        return;
    }
    const int P = d.P;
    const int per = (P + FL_CP_THREADS - 1) / FL_CP_THREADS;
    constexpr uint32_t stream = KIND == FL_COMPRESS_QSGD ? FL_QSGD_STREAM : FL_RANDK_STREAM;

    float norm = 0.f, levels = 0.f;  // qsgd
    bool as_is = false;              // qsgd: norm 0 or not finite, the update travels as it is
    unsigned thr = 0;                // randk: the k-th largest key
    int cut = 0;                     // randk: entries with that key are kept up to this dense index
    float gain = 1.f;                // randk without error feedback: P / k
    if constexpr (KIND == FL_COMPRESS_QSGD) {
        float acc = 0.f;
        for (int it = 0; it < per; it += 4) {
            float a[4], x[4], e[4];
            cp_load4(d, P, it, local, pg, ein, a, x, e);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int di = (it + i) * FL_CP_THREADS + threadIdx.x;
                if (di < P) {
                    const float u = __fadd_rn(__fsub_rn(a[i], x[i]), e[i]);
                    acc = __fadd_rn(acc, __fmul_rn(u, u));
                }
            }
        }
        // (sqrtf, not __fsqrt_rn: the intrinsic is the hardware's approximate square root unless the rounded
        // OCML operations are enabled; sqrtf is correctly rounded, fl_compress's host model depends on it)
        norm = sqrtf(block_sum_ordered<FL_CP_THREADS>(acc, wsum));
        as_is = norm == 0.f || (__float_as_uint(norm) & 0x7f800000u) == 0x7f800000u || !(norm == norm);
        levels = (float)p.levels;
        if (blockIdx.x == 0 && threadIdx.x == 0) p.stat_hist[r] = norm;
    } else {
        const int nq = (P + 3) >> 2;
        const int qper = (nq + FL_CP_THREADS - 1) / FL_CP_THREADS;  // quads per thread: t, t + 1024, ...
        for (int it = 0; it < qper; ++it) {
            const int qq = it * FL_CP_THREADS + threadIdx.x;
            if (qq < nq) {
                const uint4 o = philox4x32_10((uint32_t)qq, (uint32_t)r, (uint32_t)p.client, stream, p.key0, p.key1);
                *reinterpret_cast<uint4*>(keys + 4 * qq) = make_uint4(o.x >> 1, o.y >> 1, o.z >> 1, o.w >> 1);
            }
        }
        cp_select(keys, P, per, p.k, hist, sel, thr, cut);
        if (!p.error_feedback) gain = __fdiv_rn((float)P, (float)p.k);
        // the selection's quantile, about 1 - k / P
        if (blockIdx.x == 0 && threadIdx.x == 0) p.stat_hist[r] = __fmul_rn((float)thr, 4.656612873077392578125e-10f);
    }

    if (4 * q >= P) return;
    uint32_t wd[4] = {0u, 0u, 0u, 0u};
    if constexpr (KIND == FL_COMPRESS_QSGD) {
        const uint4 o = philox4x32_10((uint32_t)q, (uint32_t)r, (uint32_t)p.client, stream, p.key0, p.key1);
        wd[0] = o.x; wd[1] = o.y; wd[2] = o.z; wd[3] = o.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int di = 4 * q + k;
        if (di >= P) break;
        const int j = fl_image_index(d, di);
        const float x = pg[j];
        const float u = __fadd_rn(__fsub_rn(local[j], x), ein[j]);
        float c, en;
        if constexpr (KIND == FL_COMPRESS_QSGD) {
            if (as_is) {
                c = u;
                en = 0.f;
            } else {
                // (the fminf: a dominant entry whose rounded norm falls an ulp below it)
                const float a = fminf(__fmul_rn(__fdiv_rn(fabsf(u), norm), levels), levels);
                const float l = floorf(a);
                const float frac = __fsub_rn(a, l);  // exact
                const float level = (float)(wd[k] >> 8) < __fmul_rn(frac, 16777216.f) ? __fadd_rn(l, 1.f) : l;
                c = copysignf(__fdiv_rn(__fmul_rn(norm, level), levels), u);
                en = __fsub_rn(u, c);
            }
        } else {
            const unsigned key = keys[di];
            const bool kept = key > thr || (key == thr && di <= cut);
            c = kept ? __fmul_rn(u, gain) : 0.f;  // (error feedback: gain = 1, the product is u)
            en = kept ? 0.f : u;
        }
        comm[j] = __fmul_rn(w, __fadd_rn(x, c));
        eout[j] = p.error_feedback ? en : 0.f;
    }
}

static inline bool cp_is_random(int kind) { return kind == FL_COMPRESS_QSGD || kind == FL_COMPRESS_RANDK; }

// Dynamic LDS of the kernel for this model (top-k, sign: P floats; randk: P keys behind the select's
// scratch; qsgd: the scratch alone); call once before the first launch (the engine's constructor does),
// not inside a stream capture.
hipError_t fl_set_lds_limit_compress(const MLPDesc& d, int kind) {
    if (cp_is_random(kind)) {
        const size_t lds = cp_random_lds(kind, d.P);
        if (d.P < 1 || lds > (size_t)FL_LDS_DYNAMIC_MAX) return hipErrorInvalidValue;
        return hipFuncSetAttribute(kind == FL_COMPRESS_QSGD
                                       ? reinterpret_cast<const void*>(fl_compress_random_kernel<FL_COMPRESS_QSGD>)
                                       : reinterpret_cast<const void*>(fl_compress_random_kernel<FL_COMPRESS_RANDK>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    const size_t lds = (size_t)d.P * sizeof(float);
    if (d.P < 1 || lds > (size_t)FL_LDS_DYNAMIC_MAX) return hipErrorInvalidValue;  // (fits no fused kernel either)
    return hipFuncSetAttribute(reinterpret_cast<const void*>(fl_compress_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

hipError_t fl_launch_compress(const MLPDesc& d, const FLCompress& p, const float* local, const float* pg, float* comm,
                              const FLState* st, const float* rtab, hipStream_t s) {
    if ((d.Pimg & 3) != 0 || d.P < 1 || p.P != d.P || p.k < 1 || p.k > d.P || p.residual == nullptr ||
        p.stat_hist == nullptr || p.max_rounds < 1)
        return hipErrorInvalidValue;
    const int quads = (d.P + 3) / 4;
    const dim3 grid((quads + FL_CP_THREADS - 1) / FL_CP_THREADS), block(FL_CP_THREADS);
    if (cp_is_random(p.kind)) {
        const size_t lds = cp_random_lds(p.kind, d.P);
        if (lds > (size_t)FL_LDS_DYNAMIC_MAX) return hipErrorInvalidValue;
        if (p.kind == FL_COMPRESS_QSGD) {
            if (p.levels < 1 || p.levels > FL_COMPRESS_MAX_LEVELS) return hipErrorInvalidValue;
            hipLaunchKernelGGL(fl_compress_random_kernel<FL_COMPRESS_QSGD>, grid, block, lds, s, d, p, local, pg, comm,
                               st, rtab);
        } else {
            if (d.P > 65536) return hipErrorInvalidValue;  // (the tie select reads 16-bit dense indices)
            hipLaunchKernelGGL(fl_compress_random_kernel<FL_COMPRESS_RANDK>, grid, block, lds, s, d, p, local, pg, comm,
                               st, rtab);
        }
        return hipGetLastError();
    }
    if (d.P > 65536 || (size_t)d.P * sizeof(float) > (size_t)FL_LDS_DYNAMIC_MAX ||
        (p.kind != FL_COMPRESS_TOPK && p.kind != FL_COMPRESS_SIGN))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(fl_compress_kernel, grid, block, (size_t)d.P * sizeof(float), s, d, p, local, pg, comm, st, rtab);
    return hipGetLastError();
}
