// Held-out ROC AUC of the round's global model, ranked on the device.
//
// With AUC switched on, a round's held-out pair (fl_heldout.hip) is followed by two more launches that
// leave hist_u2[r][c], the doubled one-vs-rest Mann-Whitney count of class c: over (i positive, j
// negative) the sum of 2 [s_j < s_i] + [s_j == s_i], s the fp32 softmax probability of class c.  An
// exact integer: no float is ever added, so the rows are the same bits eager, replayed, on any rank.
//
//   fl_auc_keys_kernel<RT> : grid, gate and forward of fl_heldout_rows_kernel's reduce mode (stage_image,
//       stage_rows, forward_block on the fp32 master image), then per row the row mode's softmax
//       expression, one uint32 per class: keys[c][row] = (bits(s) << 1) | (y[row] == c).  s is in
//       [0, 1] or NaN; NaN becomes 0x3f800001 (the value just above 1.0), so the shift cannot overflow,
//       NaN rows tie with each other above every real probability, and the unsigned order of the keys
//       is the order by probability with the negatives of a tie group ahead of its positives.
//   fl_auc_rank_kernel : one workgroup of 1024 threads per class.  The class's n <= 32768 keys are
//       sorted in LDS and reduced to U2 without a trip through global memory.
//
// The sort is an LSD radix sort over the 31 key bits in 8-bit digits.  Wave w owns the contiguous
// segment [w seg, w seg + seg), seg = ceil(n / 16) rounded up to 64, and takes 64 keys per step; a
// thread holds its <= 32 keys in registers (k[j] = key at w seg + 64 j + lane) across a pass, so the
// scatter needs ONE key buffer: 32768 x 4 = 131072 bytes, beside 16 waves x 256 digit counters =
// 16384 bytes, 147456 of gfx950's 163840 bytes of LDS.  Per pass:
//   count   : per step the lanes find their same-digit peers with eight ballots (auc_match); the
//             first lane of each peer group adds the group's size to the wave's counter of that
//             digit.  A wave's LDS operations execute in program order, so the read-modify-write of
//             one step is complete before the next step's: no LDS atomics.
//   scan    : the 16 x 256 counters, digit-major and wave-minor, by all 1024 threads (four counters
//             each, a shuffle scan per wave, the waves' totals through LDS): counter (w, d) becomes
//             the position of wave w's first key with digit d.
//   scatter : the ballots again; key -> position = counter + (peers in lower lanes), the group's last
//             lane then advances the counter.  Stable: lower lanes, earlier steps and lower waves
//             come first.  The thread reloads its 32 keys from the sorted buffer.
// A pass whose digit is the same over all keys (the OR and the AND of the keys agree on it) is
// skipped; all four are for all-equal keys, which is why the reduction below works from registers.
//
// U2 = sum over positives p of A(p) + B(p): A(p) = negatives before p in sorted order (the negatives
// of p's own tie group are among them), B(p) = A at the first key of p's tie group (the negatives
// strictly below) = sum over tie groups of pos_g (2 neg_before_g + neg_g).  Heads of tie groups come
// from comparing key >> 1 with the neighbour's (a shuffle; the previous step's or wave's last key for
// lane 0).  Within a step A is the wave's running count plus a popcount of the negatives' ballot below
// the lane, and B the same expression at the last head at or below the lane; a group that straddles
// steps carries B forward as a wave-uniform value.  A group that straddles WAVES leaves positives
// with no head before them in their wave: each wave records (local sum, positives, positives before
// its first head, negatives, A at its last head), and one thread walks the 16 records in order, adding
// the negatives of the waves before and the carried B.  All integers, 64-bit where it matters.
//
// The round comes from the state (no per-round host argument): both launches capture into the
// round graphs.  Stores are plain vector stores; nothing is zeroed between rounds.
#define FL_FP32_DEVICE_ONLY
#include "fl_kernels.hip"
#include "fl_image.h"

#define FL_AUC_WAVES (FL_AUC_THREADS / 64)
#define FL_AUC_KPT (FL_AUC_MAX_ROWS / FL_AUC_THREADS)  // keys a thread holds at the cap
#define FL_AUC_CNT (FL_AUC_WAVES * 256)                // digit counters (uint32) ahead of the key buffer
#define FL_AUC_NAN_BITS 0x3f800001u

template <int RT>
__global__ void __launch_bounds__(FL_THREADS)
fl_auc_keys_kernel(MLPDesc d, FLAuc a, const float* __restrict__ params, const FLState* __restrict__ st) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int r;
    if (!fl_round_gate(st, a.max_rounds, r)) return;
    constexpr int R = RT * 16;
    const int row0 = blockIdx.x * R;
    const int C = d.dim[d.L];
    float* acts = lds;
    float* li = lds + d.img_lds;
    const int ylab = threadIdx.x < R ? a.y[min(row0 + (int)threadIdx.x, a.n - 1)] : 0;
    stage_image(d, params, li);
    stage_rows<RT>(a.X, a.n, d.dim[0], row0, acts + d.act_off[0], d.ld[0]);
    lds_barrier();
    forward_block<RT>(d, acts, li);
    const int row = row0 + (int)threadIdx.x;
    if (threadIdx.x < R && row < a.n) {
        const int rr = threadIdx.x;
        const float* zr = acts + d.act_off[d.L] + rr * d.ld[d.L];
        const int sr = fl_swz(rr);
        // fl_heldout_rows_kernel's row mode, expression by expression: the maximum by its first-maximum
        // scan, the denominator added in class order, exp(z - max) / sum
        float bv = zr[sr];
        for (int k = 1; k < C; ++k)
            if (zr[k ^ sr] > bv) bv = zr[k ^ sr];
        float se = 0.f;
        for (int k = 0; k < C; ++k) se = __fadd_rn(se, expf(__fsub_rn(zr[k ^ sr], bv)));
        for (int k = 0; k < C; ++k) {
            const float s = expf(__fsub_rn(zr[k ^ sr], bv)) / se;
            const uint32_t bits = s != s ? FL_AUC_NAN_BITS : __float_as_uint(s);
            a.keys[(size_t)k * a.n + row] = (bits << 1) | (ylab == k ? 1u : 0u);
        }
    }
}

// Lanes of `valid` whose 8-bit digit equals this lane's.  Every lane of the wave calls it.
__device__ __forceinline__ uint64_t auc_match(uint32_t dg, uint64_t valid) {
    uint64_t m = valid;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (dg >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// End of one unrolled step over the thread's keys.  The steps' ballots are independent of each other, and
// the scheduler would interleave all 32 for latency at the price of spilling the keys: it may not move
// instructions across this point.
__device__ __forceinline__ void auc_step_end() { __builtin_amdgcn_sched_barrier(0); }
// Start of a step: the key is made opaque to the optimiser.  The count and the scatter sweep of a pass
// take the same digits and peer masks; kept from one sweep for the other they are 3 registers per key
// (96 at the cap) next to the 32 keys, far past the 128 a thread of a 1024-thread workgroup has.
// Recomputing them is eight ballots.  (Emits no instruction.)
// The wave's key count goes the same way: the 32 steps' lane masks are loop invariants of the pass loop,
// and hoisted out of it they are 64 scalar registers held, and spilled, for the whole kernel.
__device__ __forceinline__ int auc_step_begin(uint32_t& key, int nv) {
    asm volatile("" : "+v"(key), "+s"(nv));
    return nv;
}

// lanes [0, cnt) of a wave, cnt in [0, 64]
__device__ __forceinline__ uint64_t auc_first_lanes(int cnt) { return cnt >= 64 ? ~0ull : (1ull << cnt) - 1ull; }

__global__ void __launch_bounds__(FL_AUC_THREADS)
fl_auc_rank_kernel(const uint32_t* __restrict__ keys, int n, int C, int max_rounds, const FLState* __restrict__ st,
                   unsigned long long* __restrict__ out) {
    constexpr int T = FL_AUC_THREADS, W = FL_AUC_WAVES, KPT = FL_AUC_KPT;
    extern __shared__ __attribute__((aligned(16))) uint32_t auc_lds[];
    __shared__ uint32_t orand_s[2 * W], scan_s[W], prev_s[W];
    __shared__ uint32_t rec_s[W][6];  // per wave: local sum, positives, positives before the first head, negatives, has a head, A at the last head
    if (st != nullptr) {
        int r;
        if (!fl_round_gate(st, max_rounds, r)) return;
        out += (size_t)r * C;
    }
    uint32_t* cnt = auc_lds;             // [W][256]
    uint32_t* sk = auc_lds + FL_AUC_CNT;  // [n]
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint64_t lt = (1ull << lane) - 1ull;
    keys += (size_t)blockIdx.x * n;
    const int seg = ((n + W - 1) / W + 63) & ~63;
    const int base = wave * seg;
    const int nv = min(max(n - base, 0), seg);  // keys of this wave; a wave behind a partial one has none

    uint32_t k[KPT];
    uint32_t kor = 0u, kand = ~0u;
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        // (no branch around a write to k[]: a lane past its wave's keys re-reads key n - 1 and masks it out)
        const bool valid = j * 64 + lane < nv;
        k[j] = keys[min(base + j * 64 + lane, n - 1)];
        kor |= valid ? k[j] : 0u;
        kand &= valid ? k[j] : ~0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        kor |= __shfl_xor(kor, off, 64);
        kand &= __shfl_xor(kand, off, 64);
    }
    if (lane == 0) {
        orand_s[wave] = kor;
        orand_s[W + wave] = kand;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < W; ++w) {
        kor |= orand_s[w];
        kand &= orand_s[W + w];
    }
    const uint32_t differ = kor ^ kand;  // bits on which the keys are not all alike

    volatile uint32_t* cw = cnt + wave * 256;
#pragma unroll 1
    for (int shift = 0; shift < 32; shift += 8) {
        if (((differ >> shift) & 255u) == 0u) continue;  // one digit over all keys: the order stands
#pragma unroll
        for (int q = 0; q < 4; ++q) cw[lane + 64 * q] = 0u;
#pragma unroll
        for (int j = 0; j < KPT; ++j)
            if (j * 64 < nv) {
                const uint64_t vm = auc_first_lanes(auc_step_begin(k[j], nv) - j * 64);
                const uint32_t dg = (k[j] >> shift) & 255u;
                const uint64_t m = auc_match(dg, vm);
                if (((vm >> lane) & 1ull) && (m & lt) == 0ull) cw[dg] += (uint32_t)__popcll(m);
                auc_step_end();
            }
        __syncthreads();
        {
            // flattened (digit, wave) order: thread t owns digit t >> 2, waves 4 (t & 3) .. + 3
            const int dgt = t >> 2, w0 = (t & 3) * 4;
            uint32_t v[4], s = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v[q] = cnt[(w0 + q) * 256 + dgt];
                s += v[q];
            }
            uint32_t inc = s;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t o = __shfl_up(inc, off, 64);
                if (lane >= off) inc += o;
            }
            if (lane == 63) scan_s[wave] = inc;
            __syncthreads();
            uint32_t e = inc - s;
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w < wave) e += scan_s[w];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                cnt[(w0 + q) * 256 + dgt] = e;
                e += v[q];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KPT; ++j)
            if (j * 64 < nv) {
                const uint64_t vm = auc_first_lanes(auc_step_begin(k[j], nv) - j * 64);
                const uint32_t dg = (k[j] >> shift) & 255u;
                const uint64_t m = auc_match(dg, vm);
                const uint32_t b0 = cw[dg];
                if ((vm >> lane) & 1ull) {
                    const uint32_t below = (uint32_t)__popcll(m & lt), all = (uint32_t)__popcll(m);
                    const uint32_t pos = b0 + below;
                    if (pos < (uint32_t)n) sk[pos] = k[j];
                    if (below + 1u == all) cw[dg] = b0 + all;
                }
                auc_step_end();
            }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KPT; ++j) k[j] = sk[min(auc_step_begin(k[j], base) + j * 64 + lane, n - 1)];
        // (the next scatter into sk is two barriers away: every reload is complete by then)
    }

    // the key before this wave's first: the last key of the wave before (a full one, if this wave has keys)
    {
        uint32_t wl = 0u;
#pragma unroll
        for (int j = 0; j < KPT; ++j) wl = (j + 1) * 64 == seg ? k[j] : wl;
        if (lane == 63) prev_s[wave] = wl;
    }
    __syncthreads();
    uint32_t prevk = wave > 0 ? prev_s[wave - 1] : 0u;  // wave-uniform: the key before lane 0's
    uint32_t acc = 0u;                                  // per lane: sum of A + B (wave-local) over its positives
    uint32_t negs = 0u, npos = 0u, nohead = 0u, has_head = 0u, head_a = 0u;  // wave-uniform
#pragma unroll
    for (int j = 0; j < KPT; ++j)
        if (j * 64 < nv) {
            const bool valid = j * 64 + lane < auc_step_begin(k[j], nv);
            const uint32_t up = __shfl_up(k[j], 1, 64);
            const uint32_t before = lane == 0 ? prevk : up;
            const bool first = base + j * 64 + lane == 0;
            const bool head = valid && (first || (k[j] >> 1) != (before >> 1));
            const bool positive = valid && (k[j] & 1u);
            const uint64_t hm = __ballot(head), nm = __ballot(valid && !(k[j] & 1u)), pm = __ballot(positive);
            const uint64_t hle = hm & (lt | (1ull << lane));
            const uint32_t a_loc = negs + (uint32_t)__popcll(nm & lt);
            uint32_t b_loc = head_a;
            bool hb = has_head != 0u;
            if (hle != 0ull) {
                const int hl = 63 - __clzll((long long)hle);
                b_loc = negs + (uint32_t)__popcll(nm & ((1ull << hl) - 1ull));
                hb = true;
            }
            if (positive) acc += hb ? a_loc + b_loc : a_loc;
            if (has_head == 0u)  // positives ahead of the wave's first head: their group began in an earlier wave
                nohead += (uint32_t)__popcll(pm & (hm != 0ull ? (1ull << __builtin_ctzll(hm)) - 1ull : ~0ull));
            if (hm != 0ull) {
                const int hl = 63 - __clzll((long long)hm);
                head_a = negs + (uint32_t)__popcll(nm & ((1ull << hl) - 1ull));
                has_head = 1u;
            }
            negs += (uint32_t)__popcll(nm);
            npos += (uint32_t)__popcll(pm);
            prevk = __shfl(k[j], 63, 64);
            auc_step_end();
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);  // <= 64 lanes x 32 keys x 2^16: fits
    if (lane == 0) {
        rec_s[wave][0] = acc;
        rec_s[wave][1] = npos;
        rec_s[wave][2] = nohead;
        rec_s[wave][3] = negs;
        rec_s[wave][4] = has_head;
        rec_s[wave][5] = head_a;
    }
    __syncthreads();
    if (t == 0) {
        unsigned long long u = 0ull, neg_base = 0ull, carry_b = 0ull;
        for (int w = 0; w < W; ++w) {
            const unsigned long long np = rec_s[w][1], nh = rec_s[w][2];
            // with a head before it in the wave: A and B both start at neg_base; without: B is the carried one
            u += rec_s[w][0] + neg_base * (2ull * np - nh) + carry_b * nh;
            if (rec_s[w][4]) carry_b = neg_base + rec_s[w][5];
            neg_base += rec_s[w][3];
        }
        out[blockIdx.x] = u;
    }
}

static inline size_t auc_rank_lds_bytes(int n) { return ((size_t)FL_AUC_CNT + (size_t)n) * sizeof(uint32_t); }

hipError_t fl_set_lds_limit_auc(size_t forward_bytes) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fl_auc_rank_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)auc_rank_lds_bytes(FL_AUC_MAX_ROWS));
    if (e == hipSuccess && forward_bytes != 0)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(fl_auc_keys_kernel<1>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)forward_bytes);
    if (e == hipSuccess && forward_bytes != 0)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(fl_auc_keys_kernel<2>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)forward_bytes);
    return e;
}

hipError_t fl_launch_auc_rank(const uint32_t* keys, int n, int C, int max_rounds, const FLState* st,
                              unsigned long long* out, hipStream_t s) {
    if (keys == nullptr || out == nullptr || n < 1 || n > FL_AUC_MAX_ROWS || C < 1 || C > FL_MAX_CLASSES ||
        (st != nullptr && max_rounds < 1))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(fl_auc_rank_kernel, dim3(C), dim3(FL_AUC_THREADS), auc_rank_lds_bytes(n), s, keys, n, C,
                       max_rounds, st, out);
    return hipGetLastError();
}

hipError_t fl_launch_auc_keys(const MLPDesc& d, int R, const FLAuc& p, const float* image, const FLState* st,
                              hipStream_t s) {
    const size_t fwd = (size_t)d.lds_floats * sizeof(float);
    const int C = d.dim[d.L];
    if ((R != 16 && R != 32) || p.n < 1 || p.n > FL_AUC_MAX_ROWS || p.X == nullptr || p.y == nullptr ||
        p.keys == nullptr || p.hist_u2 == nullptr || p.max_rounds < 1 || image == nullptr || st == nullptr ||
        d.L < 1 || d.L > FL_MAX_LAYERS || C < 1 || C > FL_MAX_CLASSES || fwd > (size_t)FL_LDS_DYNAMIC_MAX)
        return hipErrorInvalidValue;
    const dim3 grid((p.n + R - 1) / R);
    if (R == 16) hipLaunchKernelGGL(fl_auc_keys_kernel<1>, grid, dim3(FL_THREADS), fwd, s, d, p, image, st);
    else hipLaunchKernelGGL(fl_auc_keys_kernel<2>, grid, dim3(FL_THREADS), fwd, s, d, p, image, st);
    return hipGetLastError();
}
