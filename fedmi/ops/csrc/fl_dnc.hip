// Spectral client screening, DnC (Shejwalkar and Houmansadr, NDSS 2021, "Manipulating the Byzantine",
// Algorithm 2) in front of the aggregators: two launches per round whatever the iteration count, after the
// K clients published their contributions and before the aggregate launch.  Colluders that agree with each
// other put variance into ONE direction of update space; the rule finds that direction as the top singular
// vector of the centred update matrix and drops the clients that project most strongly onto it.  The rule is
// specified in fedmi/fl/aggregate.py (module docstring; dnc_select_ref is its model); with S the round's
// sampled clients (rtab mask), K_r = |S|, q = FLDnc::q, per iteration t:
//
//   1. R_t = the real image positions p (fl_image_lim) whose Philox word -- lane p % 4 at counter
//      (p / 4, round, t, FL_DNC_STREAM) under the seed -- is < FLDnc::thresh (thresh 0: all of them)
//   2. mu[p] = the mean over the clients of S with |v_i[p]| < FL_DNC_HUGE, added in client order from +0, one
//      division; c_i[p] = v_i[p] - mu[p]; a value that fails the test gives c_i[p] = 0 and marks client i bad
//   3. G[i][j] = sum over R_t of c_i[p] c_j[p]; a client whose G[i][i] is not finite is bad too
//   4. on the sampled clients that are not bad: w = G e_j (j: largest diagonal), 32 x (w = G w, w /= max |w|),
//      score_i = w_i^2; bad clients score +inf
//   5. the K_r - q lowest scores are kept (sortable key, ties to the lower index), bad clients never; the
//      kept word is the AND over t, ANDed with S; an empty word becomes S (the screen abstains)
//
// Both launches take the round, its liveness and the mask from `st` / rtab (fl_round_gate / fl_round_mask)
// and no per-round host argument, so they replay in a captured graph; a round that is not live writes nothing.
//
// Gram kernel.  Grid (image chunks) x iterations, 256-thread workgroups; workgroup (b, t) owns W consecutive
// image floats (fl_dnc_chunk: 256 up to 32 clients, 128 above -- the LDS budget, fl_common.h) of all K
// sources.  A thread owns one float4 column of KB / (1024 / W) rows: every global load is issued before the
// first use (rows of a gathered stack are dword-aligned only, which global dwordx4 loads accept), rows past K,
// unsampled rows and float4s past the image are never loaded and count as 0.
//   Centring on the way into LDS: the raw tile is stored, one thread per column adds its column in client
//   order (consecutive lanes, consecutive banks) and leaves mu[W]; every thread then centres what it still
//   holds in registers -- the subset test is one Philox block per float4, shared by the thread's rows -- and
//   overwrites its own slots with the centred values.  A bad value sets its row's flag (every writer stores
//   the same 1); lane i of wave 0 reads flag i and lane 0 stores the ballot: one owner, a plain store.
//   LDS tile: KB rows of W + 8 floats.  The MFMA operand read is ds_read_b128 by lane (lr, lg) at row lr,
//   float 4 lg of a 16-deep chunk.  gfx950 serves a b128 read in four groups of 16 lanes, each 8 lanes of one
//   lg and 8 of the next (rows {0-3, 12-15} with rows {4-11}), over 64 banks = 16 slots of 16 bytes: a group is
//   conflict-free iff its 16 slots (row * stride / 4 + lg) mod 16 differ.  Stride / 4 = 2 mod 16 gives
//   {0, 2, 4, 6, 8, 10, 12, 14} for the one half and the odd slots for the other, in all four groups; the
//   fp32 kernels' stride (4 mod 8 floats) needs their chunk swizzle for the same and W + 8 does not.  The
//   b128 stores (8 consecutive lanes, 32 consecutive floats of a row) and the column reads are conflict-free.
//   C C^T on v_mfma_f32_16x16x4_f32 with the k permutation of fl_kernels.hip (step j of lane group lg takes
//   k = 16 q + 4 lg + j): A lane l -> C[16 ti + (l & 15)][k], B lane l -> C[16 tj + (l & 15)][k] -- the same
//   LDS tile, so one b128 read per 16-row tile feeds four steps of every output tile it touches, and a
//   diagonal tile takes one register for both operands.  Only upper-triangle tiles: 1 / 3 / 10.
//   Work split: by k.  Wave w multiplies floats [w W / 4, (w + 1) W / 4) of the chunk into ALL output tiles
//   (<= 40 accumulator VGPRs) and the four waves' accumulators are added in wave order through LDS (the tile's
//   space, re-used behind a barrier).  Splitting by output tile would leave 3 of 4 waves idle in the 16 bucket
//   and 1 idle in the 32 bucket, and hand 10 tiles to 4 waves as 3 / 3 / 2 / 2 with every wave reading all four
//   row tiles anyway; the k split is balanced in every bucket, reads every operand once per workgroup, and its
//   cost is one 40 KB LDS round trip per workgroup.  The fold doubles as the transpose that makes the global
//   stores 64-byte runs.  No atomics, no grid barrier, no private-segment scratch.
//
// Select kernel.  One workgroup of 1024 threads: per iteration the partials are added in chunk order from +0
// (one entry per thread and trip; the order is the chunk order whatever the grid was), the upper triangle
// mirrored into the 64 x 64 LDS matrix; wave 0 then runs the rule with lane i as client i, reading G by
// columns (G is exactly symmetric -- a diagonal tile multiplies a register with itself, and a mirrored tile is
// a copy -- and lane i reading G[j][i] puts the lanes on consecutive banks), w handed round by lane reads;
// ranks by counting (fl_robust_select.h, shared with fl_screen.hip), the ballot of kept lanes.  The iteration's
// record (scores, diagonal, words, the folded matrix) goes to the scratch for tests and tools to read.
#include "fl_common.h"
#include "fl_device.h"
#include "fl_image.h"
#include "fl_philox.h"
#include "fl_robust_select.h"

#define FL_DNC_THREADS 256
#define FL_DNC_SELECT_THREADS 1024

typedef float dnc_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float dnc_f4(const float4& v, int j) {
    return j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w));
}
__device__ __forceinline__ bool dnc_ok(float x) { return fabsf(x) < FL_DNC_HUGE; }   // (false for NaN)

template <int KB>
__global__ void __launch_bounds__(FL_DNC_THREADS)
fl_dnc_gram_kernel(MLPDesc d, FLDnc p, const float* const* __restrict__ src, float* __restrict__ part,
                   const FLState* __restrict__ st) {
    constexpr int W = fl_dnc_chunk(KB), S = W + 8;
    constexpr int C4 = W / 4, RG = FL_DNC_THREADS / C4, RPT = KB / RG;   // float4 columns, row groups, rows per thread
    constexpr int RT = KB / 16, NT = RT * (RT + 1) / 2;
    constexpr int TILE = KB * S, RED = 4 * NT * 256;
    __shared__ __attribute__((aligned(16))) float lds[TILE > RED ? TILE : RED];
    __shared__ __attribute__((aligned(16))) float mu[W];
    __shared__ uint32_t badrow[KB];
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;
    const uint64_t mask = fl_round_mask(p.rtab, r, p.K);
    if (mask == 0) return;
    const int tid = threadIdx.x, t = (int)blockIdx.y;
    const int c4 = tid % C4, rg = tid / C4;
    const int p0 = (int)blockIdx.x * W + 4 * c4;
    const bool inimg = p0 < d.Pimg;   // (Pimg is a multiple of 4: a float4 is inside or outside)

    float4 v[RPT];
    bool on[RPT];
#pragma unroll
    for (int a = 0; a < RPT; ++a) {
        const int row = rg + RG * a;
        on[a] = inimg && row < p.K && ((mask >> row) & 1);
        v[a] = on[a] ? *reinterpret_cast<const float4*>(src[row] + p0) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // the float4's positions of R_t: real parameters whose Philox word is under the threshold
    const int lim = inimg ? fl_image_lim(d, p0) : 0;
    bool sel[4];
    {
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        if (p.thresh) o = philox4x32_10((uint32_t)(p0 >> 2), (uint32_t)r, (uint32_t)t, FL_DNC_STREAM, p.key0, p.key1);
        const uint32_t ow[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) sel[e] = e < lim && (p.thresh == 0 || ow[e] < p.thresh);
    }
    if (tid < KB) badrow[tid] = 0;
#pragma unroll
    for (int a = 0; a < RPT; ++a) *reinterpret_cast<float4*>(&lds[(rg + RG * a) * S + 4 * c4]) = v[a];
    __syncthreads();
    if (tid < W) {
        float s = 0.f;
        int n = 0;
        for (int i = 0; i < p.K; ++i) {
            if (!((mask >> i) & 1)) continue;   // (uniform)
            const float x = lds[i * S + tid];
            const bool ok = dnc_ok(x);
            s = ok ? __fadd_rn(s, x) : s;
            n += ok ? 1 : 0;
        }
        mu[tid] = n ? __fdiv_rn(s, (float)n) : 0.f;
    }
    __syncthreads();
    const float4 m4 = *reinterpret_cast<const float4*>(&mu[4 * c4]);
#pragma unroll
    for (int a = 0; a < RPT; ++a) {
        const float x[4] = {v[a].x, v[a].y, v[a].z, v[a].w};
        float c[4];
        bool bad = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool use = on[a] && sel[e];
            const bool ok = dnc_ok(x[e]);
            bad = bad || (use && !ok);
            c[e] = (use && ok) ? __fsub_rn(x[e], dnc_f4(m4, e)) : 0.f;
        }
        *reinterpret_cast<float4*>(&lds[(rg + RG * a) * S + 4 * c4]) = make_float4(c[0], c[1], c[2], c[3]);
        if (bad) badrow[rg + RG * a] = 1;
    }
    __syncthreads();

    // C C^T, split by k over the four waves
    const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
    dnc_f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = (dnc_f32x4){0.f, 0.f, 0.f, 0.f};
    const float* base = lds + lr * S + wave * (W / 4) + 4 * lg;
#pragma unroll
    for (int q = 0; q < W / 64; ++q) {
        float4 op[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) op[rt] = *reinterpret_cast<const float4*>(base + rt * 16 * S + 16 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int n = 0;
#pragma unroll
            for (int ti = 0; ti < RT; ++ti)
#pragma unroll
                for (int tj = ti; tj < RT; ++tj, ++n)
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(dnc_f4(op[ti], j), dnc_f4(op[tj], j), acc[n], 0, 0, 0);
        }
    }
    __syncthreads();   // every wave has read its operands: the tile's space becomes the fold's
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) lds[(wave * NT + n) * 256 + j * 64 + lane] = acc[n][j];
    __syncthreads();
    // thread (j, lane) = tid of tile n holds row 4 (lane >> 4) + j, column lane & 15 (the C/D map)
    float* out = part + ((size_t)t * gridDim.x + blockIdx.x) * fl_dnc_partial_floats(KB);
    {
        int n = 0;
#pragma unroll
        for (int ti = 0; ti < RT; ++ti)
#pragma unroll
            for (int tj = ti; tj < RT; ++tj, ++n) {
                float s = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) s = __fadd_rn(s, lds[(w * NT + n) * 256 + tid]);
                out[(16 * ti + 4 * lg + wave) * KB + 16 * tj + lr] = s;
            }
    }
    if (tid < 64) {
        const unsigned long long word = __ballot(tid < KB && badrow[tid < KB ? tid : 0] != 0);
        if (tid == 0) {
            uint32_t* bw = reinterpret_cast<uint32_t*>(out + KB * KB);
            bw[0] = (uint32_t)word;
            bw[1] = (uint32_t)(word >> 32);
        }
    }
}

__global__ void __launch_bounds__(FL_DNC_SELECT_THREADS)
fl_dnc_select_kernel(FLDnc p, int nch, float* __restrict__ scratch, unsigned long long* __restrict__ keep,
                     unsigned long long* __restrict__ hist, const FLState* __restrict__ st) {
    __shared__ float G[64 * 64];
    __shared__ uint32_t skey[64];
    __shared__ unsigned long long wbad[FL_DNC_SELECT_THREADS / 64];
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;
    const uint64_t mask = fl_round_mask(p.rtab, r, p.K);
    const int kr = __popcll(mask);
    if (kr == 0) return;
    const int tid = threadIdx.x, i = tid & 63;
    const int KB = fl_dnc_bucket(p.K), rec = fl_dnc_partial_floats(p.K);
    const bool me = tid < 64 && ((mask >> i) & 1) != 0;   // (bits >= K are cut by fl_round_mask)
    const int want = kr - p.q > 0 ? kr - p.q : 0;
    const float inf = __uint_as_float(0x7f800000u);
    float* slots = scratch + (size_t)p.iters * nch * rec;
    uint64_t kept = mask;
    for (int t = 0; t < p.iters; ++t) {
        const float* part = scratch + (size_t)t * nch * rec;
        float* slot = slots + (size_t)t * FL_DNC_SLOT;
        for (int q = tid; q < 64 * 64; q += FL_DNC_SELECT_THREADS) G[q] = 0.f;
        __syncthreads();
        // the chunk partials in chunk order from +0; the upper triangle's tiles, mirrored
        for (int q = tid; q < KB * KB; q += FL_DNC_SELECT_THREADS) {
            const int a = q / KB, c = q - a * KB;
            if ((a >> 4) > (c >> 4)) continue;
            float s = 0.f;
#pragma unroll 8
            for (int b = 0; b < nch; ++b) s = __fadd_rn(s, part[(size_t)b * rec + q]);
            G[a * 64 + c] = s;
            if ((a >> 4) != (c >> 4)) G[c * 64 + a] = s;
        }
        unsigned long long bw = 0;
        for (int b = tid; b < nch; b += FL_DNC_SELECT_THREADS) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(part + (size_t)b * rec + KB * KB);
            bw |= ((unsigned long long)w[1] << 32) | w[0];
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const uint32_t lo = __shfl_xor((int)(uint32_t)bw, off), hi = __shfl_xor((int)(uint32_t)(bw >> 32), off);
            bw |= ((unsigned long long)hi << 32) | lo;
        }
        if (i == 0) wbad[tid >> 6] = bw;
        __syncthreads();
        bool good = false;
        float score = 0.f, diag = 0.f;
        uint64_t badword = 0;
        if (tid < 64) {
            bw = 0;
#pragma unroll
            for (int w = 0; w < FL_DNC_SELECT_THREADS / 64; ++w) bw |= wbad[w];
            diag = G[i * 64 + i];
            const bool bad = me && (((bw >> i) & 1) != 0 || !(fabsf(diag) < inf));
            badword = __ballot(bad);
            good = me && !bad;
            const uint64_t gm = __ballot(good);
            // start: column j of largest diagonal among the good clients, lowest index on ties (the all-ones
            // vector is in the null space of a centred Gram matrix)
            const uint32_t dk = good ? robust_key(diag) : 0u;
            int j = 0;
            uint32_t best = 0u;
            for (int q = 0; q < p.K; ++q) {   // (lanes >= K hold no client: the loops below stop at K)
                const uint32_t kq = (uint32_t)__shfl((int)dk, q);
                if (kq > best) { best = kq; j = q; }
            }
            const int col = good ? i : 0;
            float w = good ? G[j * 64 + col] : 0.f;
            for (int step = 0; step <= FL_DNC_POWER; ++step) {
                if (step) {   // w <- G w over the good clients, in client order
                    float s = 0.f;
#pragma unroll 8
                    for (int q = 0; q < p.K; ++q) {
                        const float wq = __shfl(w, q);
                        if ((gm >> q) & 1) s = __fmaf_rn(G[q * 64 + col], wq, s);   // (uniform)
                    }
                    w = good ? s : 0.f;
                }
                float mx = fabsf(w);
#pragma unroll
                for (int off = 32; off; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
                if (mx > 0.f) w = __fdiv_rn(w, mx);   // a zero vector stays zero
            }
            score = good ? __fmul_rn(w, w) : (me ? inf : 0.f);
            skey[i] = me ? robust_key(score) : 0xffffffffu;   // an unsampled lane ranks behind every sampled one
        }
        __syncthreads();
        if (tid < 64) {
            const uint64_t kt = __ballot(good && robust_rank64(skey, i) < want);
            kept &= kt;
            slot[i] = score;
            slot[64 + i] = diag;
            if (i == 0) {
                uint32_t* w = reinterpret_cast<uint32_t*>(slot + 128);
                w[0] = (uint32_t)kt; w[1] = (uint32_t)(kt >> 32);
                w[2] = (uint32_t)badword; w[3] = (uint32_t)(badword >> 32);
            }
        }
        for (int q = tid; q < 64 * 64; q += FL_DNC_SELECT_THREADS) slot[192 + q] = G[q];
        __syncthreads();   // G and skey are rewritten by the next iteration
    }
    if (tid == 0) {
        if (kept == 0) kept = mask;   // nobody survives: the screen abstains, as multi-Krum does where it is undefined
        *keep = kept;
        hist[r] = kept;
    }
}

template <int KB>
static void dnc_gram_launch(const MLPDesc& d, const FLDnc& p, const float* const* src, float* scratch,
                            const FLState* st, hipStream_t s) {
    hipLaunchKernelGGL((fl_dnc_gram_kernel<KB>), dim3(fl_dnc_chunks(d.Pimg, p.K), p.iters), dim3(FL_DNC_THREADS), 0, s,
                       d, p, src, scratch, st);
}

static bool dnc_args_ok(const FLDnc& p) {
    return p.rtab != nullptr && p.K >= 1 && p.K <= FL_DNC_MAX_K && p.max_rounds >= 1 && p.f >= 0 && p.q >= 0 &&
           p.iters >= 1 && p.iters <= FL_DNC_MAX_ITERS;
}

hipError_t fl_launch_dnc_gram(const MLPDesc& d, const FLDnc& p, const float* const* src, float* scratch,
                              const FLState* st, hipStream_t s) {
    if ((d.Pimg & 3) != 0 || d.Pimg < 4 || src == nullptr || scratch == nullptr || st == nullptr || !dnc_args_ok(p))
        return hipErrorInvalidValue;
    const int kb = fl_dnc_bucket(p.K);
    if (kb == 16) dnc_gram_launch<16>(d, p, src, scratch, st, s);
    else if (kb == 32) dnc_gram_launch<32>(d, p, src, scratch, st, s);
    else dnc_gram_launch<64>(d, p, src, scratch, st, s);
    return hipGetLastError();
}

hipError_t fl_launch_dnc_select(const MLPDesc& d, const FLDnc& p, float* scratch, unsigned long long* keep,
                                unsigned long long* hist, const FLState* st, hipStream_t s) {
    if ((d.Pimg & 3) != 0 || d.Pimg < 4 || scratch == nullptr || keep == nullptr || hist == nullptr || st == nullptr ||
        !dnc_args_ok(p))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(fl_dnc_select_kernel, dim3(1), dim3(FL_DNC_SELECT_THREADS), 0, s, p, fl_dnc_chunks(d.Pimg, p.K),
                       scratch, keep, hist, st);
    return hipGetLastError();
}
