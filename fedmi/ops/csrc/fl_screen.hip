// Multi-Krum client screening in front of the aggregators (Blanchard et al. 2017, "Machine Learning
// with Adversaries: Byzantine Tolerant Gradient Descent"): two launches per round, after the K
// clients published their contributions (the unscaled post-step local models, as for fl_robust) and
// before the aggregate launch, decide from pairwise WHOLE-MODEL distances which of the round's
// sampled clients the coordinate rule may use.  With S_r the sampled clients (rtab mask of the
// round in `st`), K_r = |S_r|, f = FLScreen::f the Byzantine clients assumed and v_k client k's image:
//
//   1. d(i, j) = sum over the real parameters p of the image of (v_i[p] - v_j[p])^2, i != j in S_r;
//      d(i, i) = 0; a sum that is not < +inf (NaN, inf, overflow) is +inf
//   2. K_r < 2 f + 3: all of S_r is kept.  Otherwise score(i) = the sum of the nb = K_r - f - 2
//      smallest d(i, j), j in S_r \ {i} (ties by client index), added in client order from 0
//   3. the m_r = min(m, K_r - f) clients of smallest score are kept (ties, +inf == +inf included,
//      to the lower client index; compared on the sortable key of fl_robust_select.h)
//
// fl_robust then runs over the kept set: it ANDs the kept mask into the round's mask (its `keep`
// argument), so K_r becomes m_r in the trim count and in the divisor.  Every operation is an explicit
// round-to-nearest fp32 intrinsic and every sum has ONE order, so the kept set is bit-identical on
// every rank and across replays; fedmi/fl/aggregate.py pair_distances_model / screen_select are the
// host models.  A round that is not live writes nothing here (neither the matrix, the kept mask nor
// the history) and fl_robust folds it as ever.  Neither launch takes a per-round host argument.
//
// Distance kernel.  256-thread workgroups; a workgroup owns a T x T tile of client pairs of the upper
// triangle (tile row <= tile column) and walks the image once: thread t takes the float4s t, t + 256,
// ... in increasing order, loads that float4 of the tile's 2 T source rows -- every load issued
// before the first use -- and adds sub / mul / add per lane x, y, z, w into one register accumulator
// per pair (image padding adds +0: fl_image_lim, so what a peer writes into padding moves no score).
// Each pair's 256 partial sums are then added by block_sum_ordered: the wave xor tree, the four wave
// sums in wave order.  A pair's sum therefore depends on the two images alone -- not on K, the grid or
// the tile size.  a - b and b - a square to the same float, so the lower triangle is the mirror of the
// upper one, stored by the same workgroup.  No atomics, no grid barrier, no LDS beyond the wave sums,
// plain vector stores.  Tiles without a sampled pair return at once.
//
// Select kernel.  One wave; lane i is client i (K <= 64, the rtab mask width).  The matrix and its
// sortable keys are staged in LDS (2 x 16 KB at K = 64) and read by columns -- d is exactly symmetric,
// and lane i reading d[j][i] puts the 64 lanes on consecutive banks where row reads would all hit one.
// Each lane ranks its row by counting (K^2 key reads per lane, branch-free so the reads pipeline: entries
// that are no distance between two sampled clients carry the key above every value's), adds its nb
// nearest in client order, the scores are ranked across lanes through LDS the same way, and lane 0
// writes the ballot of kept lanes to `keep` and to screen_hist[round].
#include "fl_common.h"
#include "fl_device.h"
#include "fl_image.h"
#include "fl_robust_select.h"

#define FL_SCREEN_THREADS 256

template <int T>
__global__ void __launch_bounds__(FL_SCREEN_THREADS)
fl_screen_dist_kernel(MLPDesc d, FLScreen p, const float* const* __restrict__ src, float* __restrict__ dist,
                      const FLState* __restrict__ st, int tiles) {
    __shared__ float wsum[T * T][FL_SCREEN_THREADS / 64];
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;
    const uint64_t mask = fl_round_mask(p.rtab, r, p.K);
    // tile (ti, tj), ti <= tj, of the upper triangle: workgroup b counts them row by row
    int ti = 0, b = (int)blockIdx.x;
    while (b >= tiles - ti) { b -= tiles - ti; ++ti; }
    const int tj = ti + b;
    const int i0 = ti * T, j0 = tj * T;
    const uint64_t tile_bits = (1ull << T) - 1ull;   // (T <= 8)
    if (((mask >> i0) & tile_bits) == 0 || ((mask >> j0) & tile_bits) == 0) return;
    if constexpr (T == 1) {
        // a diagonal 1 x 1 tile is d(i, i) = 0: nothing to read.  (A diagonal tile of T >= 2 still walks its
        // T (T - 1) / 2 distinct pairs; it computes each from both sides, one pass of the same loads.)
        if (ti == tj) {
            if (threadIdx.x == 0) dist[(size_t)i0 * p.K + i0] = 0.f;
            return;
        }
    }

    const float* ra[T];
    const float* rb[T];
#pragma unroll
    for (int a = 0; a < T; ++a) {   // slots past K re-read source K - 1 and are not stored
        ra[a] = src[i0 + a < p.K ? i0 + a : p.K - 1];
        rb[a] = src[j0 + a < p.K ? j0 + a : p.K - 1];
    }
    float acc[T][T];
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int c = 0; c < T; ++c) acc[a][c] = 0.f;

    const int n4 = d.Pimg >> 2;
    // (float4 loads: a source is 16-byte aligned when it is a buffer of its own; a row of a gathered
    // stack starts Pimg + tails floats after the last and may be dword-aligned only, which gfx950's
    // global dwordx4 loads accept -- fl_robust reads the same rows the same way)
    for (int q = threadIdx.x; q < n4; q += FL_SCREEN_THREADS) {
        float4 va[T], vb[T];
#pragma unroll
        for (int a = 0; a < T; ++a) va[a] = reinterpret_cast<const float4*>(ra[a])[q];
#pragma unroll
        for (int a = 0; a < T; ++a) vb[a] = reinterpret_cast<const float4*>(rb[a])[q];
        const int lim = fl_image_lim(d, 4 * q);   // lanes e < lim are real parameters
#pragma unroll
        for (int a = 0; a < T; ++a)
#pragma unroll
            for (int c = 0; c < T; ++c) {
                const float x[4] = {va[a].x, va[a].y, va[a].z, va[a].w};
                const float y[4] = {vb[c].x, vb[c].y, vb[c].z, vb[c].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float df = __fsub_rn(x[e], y[e]);
                    const float sq = __fmul_rn(df, df);
                    acc[a][c] = __fadd_rn(acc[a][c], e < lim ? sq : 0.f);
                }
            }
    }
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int c = 0; c < T; ++c) acc[a][c] = block_sum_ordered<FL_SCREEN_THREADS>(acc[a][c], wsum[a * T + c]);
    if (threadIdx.x != 0) return;
    const float inf = __uint_as_float(0x7f800000u);
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int c = 0; c < T; ++c) {
            const int i = i0 + a, j = j0 + c;
            if (i >= p.K || j >= p.K) continue;
            const float v = i == j ? 0.f : (acc[a][c] < inf ? acc[a][c] : inf);
            dist[(size_t)i * p.K + j] = v;
            dist[(size_t)j * p.K + i] = v;
        }
}

__global__ void __launch_bounds__(64)
fl_screen_select_kernel(FLScreen p, const float* __restrict__ dist, unsigned long long* __restrict__ keep,
                        unsigned long long* __restrict__ hist, const FLState* __restrict__ st) {
    __shared__ float D[FL_SCREEN_MAX_K * FL_SCREEN_MAX_K];
    __shared__ uint32_t KEY[FL_SCREEN_MAX_K * FL_SCREEN_MAX_K];
    __shared__ uint32_t skey[64];
    int r;
    if (!fl_round_gate(st, p.max_rounds, r)) return;
    const uint64_t mask = fl_round_mask(p.rtab, r, p.K);
    const int K = p.K, i = threadIdx.x;
    const int kr = __popcll(mask);
    if (kr == 0) return;
    uint64_t kept = mask;
    if (kr >= 2 * p.f + 3) {   // (uniform: mask, f are the launch's)
        // the matrix and its sortable keys; an entry that is no distance between two different sampled
        // clients gets the key above every value's, so the counting loops below need no branch for it
        const uint32_t none = 0xffffffffu;
        for (int q = i; q < K * K; q += 64) {
            const int a = q / K, c = q - a * K;
            const float v = dist[q];
            D[q] = v;
            KEY[q] = (a != c && ((mask >> a) & 1) && ((mask >> c) & 1)) ? robust_key(v) : none;
        }
        __syncthreads();
        const bool me = ((mask >> i) & 1) != 0;   // (bits >= K are cut by fl_round_mask)
        const int col = me ? i : 0;               // lanes that are no sampled client read column 0 and drop it
        const int nb = kr - p.f - 2;
        float score = 0.f;
        for (int j = 0; j < K; ++j) {
            if (!((mask >> j) & 1)) continue;     // (uniform)
            const uint32_t kj = KEY[j * K + col];  // d(i, j), read down the column
            const float dj = D[j * K + col];
            int rank = 0;
#pragma unroll 8
            for (int q = 0; q < K; ++q) {
                const uint32_t kq = KEY[q * K + col];
                rank += (kq < kj || (kq == kj && q < j)) ? 1 : 0;
            }
            score = (kj != none && rank < nb) ? __fadd_rn(score, dj) : score;
        }
        skey[i] = me ? robust_key(score) : none;   // an unsampled lane ranks behind every sampled one
        __syncthreads();
        const int want = p.m > 0 && p.m < kr - p.f ? p.m : kr - p.f;
        int rank = 0;
        const uint32_t ki = skey[i];
#pragma unroll 8
        for (int q = 0; q < 64; ++q) {
            const uint32_t kq = skey[q];
            rank += (q != i && (kq < ki || (kq == ki && q < i))) ? 1 : 0;
        }
        kept = __ballot(me && rank < want);
    }
    if (i == 0) {
        *keep = kept;
        hist[r] = kept;
    }
}

template <int T>
static void screen_dist_launch(const MLPDesc& d, const FLScreen& p, const float* const* src, float* dist,
                               const FLState* st, hipStream_t s) {
    const int tiles = (p.K + T - 1) / T;
    hipLaunchKernelGGL((fl_screen_dist_kernel<T>), dim3(tiles * (tiles + 1) / 2), dim3(FL_SCREEN_THREADS), 0, s, d, p,
                       src, dist, st, tiles);
}

hipError_t fl_launch_screen_dist(const MLPDesc& d, const FLScreen& p, const float* const* src, float* dist,
                                 const FLState* st, hipStream_t s, int tile) {
    if ((d.Pimg & 3) != 0 || d.Pimg < 4 || src == nullptr || dist == nullptr || st == nullptr || p.rtab == nullptr ||
        p.K < 1 || p.K > FL_SCREEN_MAX_K || p.max_rounds < 1)
        return hipErrorInvalidValue;
    if (tile == 0) tile = fl_screen_tile(p.K);
    if (tile == 1) screen_dist_launch<1>(d, p, src, dist, st, s);
    else if (tile == 2) screen_dist_launch<2>(d, p, src, dist, st, s);
    else if (tile == 4) screen_dist_launch<4>(d, p, src, dist, st, s);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t fl_launch_screen_select(const FLScreen& p, const float* dist, unsigned long long* keep,
                                   unsigned long long* hist, const FLState* st, hipStream_t s) {
    if (dist == nullptr || keep == nullptr || hist == nullptr || st == nullptr || p.rtab == nullptr || p.K < 1 ||
        p.K > FL_SCREEN_MAX_K || p.max_rounds < 1 || p.f < 0 || p.m < 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(fl_screen_select_kernel, dim3(1), dim3(64), 0, s, p, dist, keep, hist, st);
    return hipGetLastError();
}
