// Sequence scoring (include/omnibiote_hip_score.h): the readout product x W^T fused with its log-softmax.  The readout is the one
// product here whose output is only ever reduced along N, so the (R, V) logits never exist: a workgroup owns one 128-row tile of x
// and one contiguous slice of the vocabulary and walks the slice's 128-column tiles of w.
//   tile body   gemm_bf16_v1.hip's: 128 x 128 tile, 4 waves at 64 x 64, v_mfma_f32_16x16x32_bf16 with the operands swapped, K step 64,
//               two LDS stages filled by LDS-DMA (hardware zero fill past the tensors' ends), the XOR swizzle, the same half-tile
//               software pipeline.  The x tile is streamed again (from L2) for every tile of w.
//   after it    acc * alpha -> bf16 -> LDS, as v1's epilogue stages it.  Thread t then owns row t >> 1 and the 64-column half t & 1
//               of the staged tile: it masks columns >= V to -inf (the DMA zero-fills those rows of w, and a zero logit is not an
//               absent one), folds the 64 values into its running (max, sum) — registers, across the whole slice — and looks
//               at its share of the row's targets: one that lies in this tile is read from the staged tile into logits_at.
//   per slice   the two halves of a row are combined (half 0, then half 1) and the pair is written to ws[row][slice].
// A second launch, one thread per row, combines the pairs in slice order into lse and writes logprobs (and both outputs of the
// targets that are -1 or out of range).  Which lane holds a row depends on the row's place in its tile, the order of every sum does not:
// a row's bits do not depend on R or on the other rows.
//
// The fused draw (include/omnibiote_hip_fill.h: obte_readout_sample_bf16) is the same body compiled with SampleParams: the staged value
// becomes y = z inv_temp (-inf for a column the row's bit mask excludes), the (max, sum) runs over y unchanged, and each thread also
// keeps a running best (y + Gumbel noise, column, y) of its columns — visited in ascending order, replaced on a strictly larger value,
// so equal values stay with the smaller column.  The halves and then the slices fold their bests under that same total order.
// obte_fill_commit, the unmasking loop's bookkeeping, is at the end of this file.
#include <math.h>
#include "gemm_common.h"
#include "../../include/omnibiote_hip_score.h"
#include "../../include/omnibiote_hip_fill.h"

namespace obte_score {

using obte_gemm_v2::kmaj_off;
using obte_gemm_v2::xcd_remap;

constexpr int BM = 128, BN = 128, BKT = 64;
constexpr int TILE_BYTES = 128 * 64 * 2;      // one operand tile
constexpr int STAGE_BYTES = 2 * TILE_BYTES;   // x + w
constexpr int SMEM_BYTES = 2 * STAGE_BYTES;   // two stages = 64 KiB -> 2 workgroups per CU
constexpr int EPI_LD = 144;                   // bytes per staged row of a wave's 64 x 64 quarter: 64 bf16 + 16 B pad
constexpr int EPI_WAVE_BYTES = 64 * EPI_LD;
constexpr int MAX_SLICES = 64, MAX_K = 64;
constexpr float LOG2E = 1.4426950408889634f;

struct ScoreParams {
    static constexpr bool SAMPLE = false;
    const bf16* x; const bf16* w; const int32_t* targets; float* logits_at; float2* part;
    int64_t R, V, C, ldx, ldw, K;
    int64_t x_elems, w_elems;
    int tiles_m, tiles_n, slices;
    float alpha;
};

struct Best { float p; int32_t col; float y; };   // a perturbed value, its column, y at that column

struct SampleParams {
    static constexpr bool SAMPLE = true;
    const bf16* x; const bf16* w; const int64_t* keys; const uint8_t* allowed; float2* part; Best* best;
    int64_t R, V, C, ldx, ldw, allowed_ld;
    int64_t x_elems, w_elems;
    int tiles_m, tiles_n, slices;
    float alpha, inv_temp;   // inv_temp as the kernel multiplies by it: 1 in a greedy call
    int greedy;
    DropCfg noise;
};

// per-lane byte offsets (relative to the tile origin in global memory) of the four LDS-DMA pieces a lane issues (v1's k-contiguous form)
__device__ __forceinline__ void dma_offsets(int wave, int lane, int64_t ld, int (&voff)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (i * 4 + wave) * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ ((row >> 1) & 7);
        voff[i] = (int)((row * ld + chunk * 8) * 2);
    }
}

__device__ __forceinline__ void dma_tile(const bf16* origin, int64_t elems_left, const int (&voff)[4], char* lds_tile, int wave) {
    const i32x4_t rsrc = make_rsrc_words(origin, elems_left * 2);
    const uint32_t base = lds_addr_of(lds_tile) + wave * 1024;
#pragma unroll
    for (int i = 0; i < 4; ++i) lds_dma16(rsrc, base + i * 4 * 1024, voff[i]);
}

__device__ __forceinline__ bf16x8 load_frag(const char* tile, int mn0, int s, int lane) {
    return *reinterpret_cast<const bf16x8*>(tile + kmaj_off(mn0 + (lane & 15), 4 * s + (lane >> 4)));
}

// one rounded operation each, never fused into a neighbour (hipcc contracts a * b + c by default, and not alike in every kernel)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

__device__ __forceinline__ float exp2_of(float d) { return __builtin_amdgcn_exp2f(d * LOG2E); }   // e^d; d = -inf gives 0

// (m, s) <- (m, s) and (m2, s2), in that order; s counts in units of e^m.  No inf - inf: an all -inf side scales by e^(-inf - 0) = 0.
// Two rounded products and their sum, written out: the score's and the draw's combine kernels round alike.
__device__ __forceinline__ void fold_pair(float& m, float& s, float m2, float s2) {
    const float mx = fmaxf(m, m2);
    const float ms = mx == -INFINITY ? 0.f : mx;
    s = add_rn(mul_rn(s, exp2_of(m - ms)), mul_rn(s2, exp2_of(m2 - ms)));
    m = mx;
}

// the rule's g = -ln(-ln(1 - w)), w = (h + 0.5) 2^-32, in fp32.  w and 1 - w are each formed from the integer (h and ~h = 2^32 - 1 - h), so
// both carry a relative error of 2^-23 at most however close to 0 or 1 they lie; E = -ln(1 - w) is the logarithm where that leaves it a
// small relative error (w >= 1/16: E >= 0.0645) and the series w + w^2/2 + ... + w^6/6 below (remainder below 2^-26 E).  E lies in
// [2^-33, 22.9]: g is finite for every h.
__device__ __forceinline__ float gumbel_of(uint32_t h) {
    constexpr float LN2 = 0.6931471805599453f;
    const float w = ((float)h + 0.5f) * 0x1p-32f;
    const float u = ((float)~h + 0.5f) * 0x1p-32f;
    const float ser = w * (1.f + w * (0.5f + w * (0.33333334f + w * (0.25f + w * (0.2f + w * 0.16666667f)))));
    const float lg = -LN2 * __builtin_amdgcn_logf(u);
    const float e = w < 0.0625f ? ser : lg;
    return -LN2 * __builtin_amdgcn_logf(e);
}

// a <- the better of a and b: the larger value, the smaller column among equal values; an empty best (col < 0, p = -inf) never wins
__device__ __forceinline__ void fold_best(Best& a, const Best& b) {
    if (b.col >= 0 && (a.col < 0 || b.p > a.p || (b.p == a.p && b.col < a.col))) a = b;
}

template <class P>
__device__ __forceinline__ void readout_body(const P& p) {
    constexpr bool SAMPLE = P::SAMPLE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;

    // workgroup -> (row tile, slice): the workgroups of one XCD (own L2) take consecutive row tiles of one slice, so a tile of w is read
    // from memory once per XCD
    const int wgid = xcd_remap(blockIdx.x, p.tiles_m * p.slices);
    const int tm = wgid % p.tiles_m, sl = wgid / p.tiles_m;
    const int t_begin = (int)((int64_t)sl * p.tiles_n / p.slices), t_end = (int)((int64_t)(sl + 1) * p.tiles_n / p.slices);
    const int64_t m0 = (int64_t)tm * BM;

    int voff_a[4], voff_b[4];
    dma_offsets(wave, lane, p.ldx, voff_a);
    dma_offsets(wave, lane, p.ldw, voff_b);
    const int wm = wave >> 1, wn = wave & 1;
    const int nk = (int)(p.C / BKT);

    // this thread's part in the reduction: row srow of the tile, columns [64 shalf, 64 shalf + 64)
    const int srow = threadIdx.x >> 1, shalf = threadIdx.x & 1;
    const int64_t grow = m0 + srow;
    const bool row_ok = grow < p.R;
    const char* my_rows = smem + (srow >> 6) * 2 * EPI_WAVE_BYTES + (srow & 63) * EPI_LD;   // + (column >> 6) * EPI_WAVE_BYTES + (column & 63) * 2
    float run_m = -INFINITY, run_s = 0.f, run_c = 0.f;   // the row half's maximum, the sum of e^(z - maximum), what the sum's additions lost
    int K = 0, tg0 = -1;
    if constexpr (!SAMPLE) {
        K = (int)p.K;
        tg0 = row_ok && shalf < K ? p.targets[grow * K + shalf] : -1;   // targets k = shalf, shalf + 2, ...: the first stays in a register
    }
    // the draw: this row's key for the noise, its bit mask (none for a row past R: its results go nowhere) and the running best
    uint32_t rowkey = 0;
    const uint8_t* mrow = nullptr;
    Best best = {-INFINITY, -1, -INFINITY};
    if constexpr (SAMPLE) {
        if (row_ok) {
            if (!p.greedy) rowkey = drop_rowkey((uint64_t)(p.keys ? p.keys[grow] : grow), p.noise);
            if (p.allowed) mrow = p.allowed + grow * p.allowed_ld;
        }
    }

    for (int tn = t_begin; tn < t_end; ++tn) {
        const int64_t n0 = (int64_t)tn * BN;
        f32x4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

        auto issue = [&](int t, int stage) {
            const int64_t k0 = (int64_t)t * BKT;
            const int64_t ao = m0 * p.ldx + k0, bo = n0 * p.ldw + k0;
            char* st = smem + stage * STAGE_BYTES;
            dma_tile(p.x + ao, p.x_elems - ao, voff_a, st, wave);
            dma_tile(p.w + bo, p.w_elems - bo, voff_b, st + TILE_BYTES, wave);
        };
        // ---- main loop, v1's: software pipelined over half K-tiles ---------------------------------------------------------------
        //   step t:  read F1(t) | MFMA F0(t) | wait tile t+1, barrier | read F0(t+1), issue DMA of tile t+2 | MFMA F1(t)
        auto load_frags = [&](int t, int ks, bf16x8 (&af)[4], bf16x8 (&bfr)[4]) {
            const char* ta = smem + (t & 1) * STAGE_BYTES;
            const char* tb = ta + TILE_BYTES;
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = load_frag(ta, wm * 64 + i * 16, ks, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i) bfr[i] = load_frag(tb, wn * 64 + i * 16, ks, lane);
        };
        auto mma = [&](const bf16x8 (&af)[4], const bf16x8 (&bfr)[4]) {
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    // operands swapped: the accumulator holds C^T (row = n, col = m)
                    acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[ni][mi], 0, 0, 0);
        };
        bf16x8 a0[4], b0[4], a1[4], b1[4];
        issue(0, 0);
        if (nk > 1) {
            issue(1, 1);
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // tile 0 landed; the 8 pieces of tile 1 stay in flight
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        load_frags(0, 0, a0, b0);
        for (int t = 0; t + 1 < nk; ++t) {
            load_frags(t, 1, a1, b1);
            __builtin_amdgcn_sched_barrier(0);
            mma(a0, b0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0x0070);   // vmcnt(0) lgkmcnt(0): tile t+1 landed, F1(t) in registers
            __builtin_amdgcn_s_barrier();
            load_frags(t + 1, 0, a0, b0);
            if (t + 2 < nk) issue(t + 2, t & 1);  // the stage every wave has just finished reading
            __builtin_amdgcn_sched_barrier(0);
            mma(a1, b1);
            __builtin_amdgcn_sched_barrier(0);
        }
        load_frags(nk - 1, 1, a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        mma(a0, b0);
        mma(a1, b1);
        __syncthreads();

        // the draw: the mask bits of this thread's 64 columns, byte by byte (a row's mask may start at any address) and none beyond the
        // row's ceil(V / 8); asked for here, with no DMA piece in flight, they arrive under the staging
        uint32_t mbits0 = ~0u, mbits1 = ~0u;
        if constexpr (SAMPLE) {
            if (mrow) {
                const int64_t byte0 = (n0 + shalf * 64) >> 3, nbytes = (p.V + 7) >> 3;
                mbits0 = 0; mbits1 = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (byte0 + j < nbytes) mbits0 |= (uint32_t)mrow[byte0 + j] << (8 * j);
                    if (byte0 + 4 + j < nbytes) mbits1 |= (uint32_t)mrow[byte0 + 4 + j] << (8 * j);
                }
            }
        }

        // ---- acc * alpha -> bf16 -> LDS (per-wave 64 x 64 quarter), v1's staging ------------------------------------------------------
        char* stg = smem + wave * EPI_WAVE_BYTES;
        const int em = lane & 15, en = (lane >> 4) * 4;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                bf16x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = f2bf(acc[ni][mi][r] * p.alpha);
                *reinterpret_cast<bf16x4*>(stg + (mi * 16 + em) * EPI_LD + (ni * 16 + en) * 2) = v;
            }
        __syncthreads();

        // ---- the row's 64 staged values of this half into the running (max, sum) ------------------------------------------------------
        bf16x8 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const bf16x8*>(my_rows + shalf * EPI_WAVE_BYTES + j * 16);
        const int64_t left = p.V - (n0 + shalf * 64);            // columns of this half below V
        const int lim = left >= 64 ? 64 : (left < 0 ? 0 : (int)left);
        float tmax = -INFINITY;
        float y[SAMPLE ? 64 : 1];   // the draw: y = z inv_temp, -inf at a column past V or one the mask excludes
        if constexpr (SAMPLE) {
            const uint64_t keep = (lim == 64 ? ~0ull : (1ull << lim) - 1ull) & (((uint64_t)mbits1 << 32) | mbits0);
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int c = j * 8 + e;
                    y[c] = (keep >> c) & 1 ? mul_rn(bf2f(v[j][e]), p.inv_temp) : -INFINITY;
                    tmax = fmaxf(tmax, y[c]);
                }
        } else if (lim == 64) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) tmax = fmaxf(tmax, bf2f(v[j][e]));
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) tmax = fmaxf(tmax, j * 8 + e < lim ? bf2f(v[j][e]) : -INFINITY);
        }
        // the tile's own sum first — eight chains of eight, then a tree — and that into the running sum with its rounding error carried
        // along (two-sum): one chain over the slice's thousands of terms drifts, the more so when the logits take few distinct values
        const float mnew = fmaxf(run_m, tmax);
        const float ms = mnew == -INFINITY ? 0.f : mnew;
        float ps[8];
        if constexpr (SAMPLE) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                ps[j] = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) ps[j] += exp2_of(y[j * 8 + e] - ms);   // e^(-inf) = 0: an excluded column adds nothing
            }
        } else if (lim == 64) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                ps[j] = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) ps[j] += exp2_of(bf2f(v[j][e]) - ms);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                ps[j] = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) ps[j] += j * 8 + e < lim ? exp2_of(bf2f(v[j][e]) - ms) : 0.f;
            }
        }
        const float tsum = ((ps[0] + ps[1]) + (ps[2] + ps[3])) + ((ps[4] + ps[5]) + (ps[6] + ps[7]));
        // (which products fuse into the additions is written out — it is the form this sum has always had — so that the score and the
        // draw, two kernels built from this body, round alike: a greedy draw's lse has the score's bits)
        const float f = exp2_of(run_m - ms);   // 1 unless the maximum moved
        const float s_old = mul_rn(run_s, f);
        const float s_new = __fmaf_rn(run_s, f, tsum);
        const float lost = s_old >= tsum ? add_rn(__fmaf_rn(run_s, f, -s_new), tsum) : __fmaf_rn(run_s, f, sub_rn(tsum, s_new));
        run_c = __fmaf_rn(run_c, f, lost);
        run_s = s_new;
        run_m = mnew;

        // ---- the draw: this thread's 64 columns in ascending order against its running best ---------------------------------------------
        if constexpr (SAMPLE) {
            const uint32_t col0 = (uint32_t)(n0 + shalf * 64);
            if (p.greedy) {
#pragma unroll
                for (int c = 0; c < 64; ++c)
                    if (y[c] > best.p) best = {y[c], (int32_t)(col0 + c), y[c]};
            } else {
#pragma unroll
                for (int c = 0; c < 64; ++c) {
                    const float pv = y[c] + gumbel_of(obte_hash32(rowkey ^ (col0 + c)));   // -inf stays -inf: the noise is finite
                    if (pv > best.p) best = {pv, (int32_t)(col0 + c), y[c]};
                }
            }
        }

        // ---- targets of this row that lie in this tile --------------------------------------------------------------------------------
        if constexpr (!SAMPLE) if (row_ok) {
            const int64_t nend = n0 + BN < p.V ? n0 + BN : p.V;
            auto take = [&](int k, int tg) {
                if (tg >= n0 && tg < nend) {
                    const int c = (int)(tg - n0);
                    const bf16 z = *reinterpret_cast<const bf16*>(my_rows + (c >> 6) * EPI_WAVE_BYTES + (c & 63) * 2);
                    p.logits_at[grow * K + k] = bf2f(z);
                }
            };
            take(shalf, tg0);
            for (int k = shalf + 2; k < K; k += 2) take(k, p.targets[grow * K + k]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the counted waits of the next tile's loop see its DMA pieces alone
        __syncthreads();                                    // the staged tile is read: the stages may be filled again
    }

    // ---- one (max, sum) per row and slice: half 0, then half 1 ----------------------------------------------------------------------------
    const float mine = run_s + run_c;
    const float om = __shfl_xor(run_m, 1, 64), os = __shfl_xor(mine, 1, 64);
    if (row_ok && shalf == 0) {   // (the fused form written out, as above)
        const float m = fmaxf(run_m, om);
        const float ms = m == -INFINITY ? 0.f : m;
        const float s = __fmaf_rn(mine, exp2_of(run_m - ms), mul_rn(os, exp2_of(om - ms)));
        p.part[grow * p.slices + sl] = make_float2(m, s);
    }
    if constexpr (SAMPLE) {
        const Best other = {__shfl_xor(best.p, 1, 64), __shfl_xor(best.col, 1, 64), __shfl_xor(best.y, 1, 64)};
        fold_best(best, other);
        if (row_ok && shalf == 0) p.best[grow * p.slices + sl] = best;
    }
}

__global__ __launch_bounds__(256, 2) void readout_score_kernel(ScoreParams p) { readout_body(p); }
__global__ __launch_bounds__(256, 2) void readout_sample_kernel(SampleParams p) { readout_body(p); }

// one thread per row: the slices' pairs in slice order -> lse, the slices' bests -> the token; logprob = y[token] - lse
__global__ __launch_bounds__(256) void readout_sample_combine_kernel(const float2* part, const Best* bests, int slices, int32_t* tokens, float* logprob,
                                                                     float* lse, int64_t R) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float m = -INFINITY, s = 0.f;
    Best best = {-INFINITY, -1, -INFINITY};
    for (int i = 0; i < slices; ++i) {
        const float2 q = part[r * slices + i];
        fold_pair(m, s, q.x, q.y);
        fold_best(best, bests[r * slices + i]);
    }
    const float l = (m == -INFINITY ? 0.f : m) + logf(s);
    lse[r] = l;
    tokens[r] = best.col;
    logprob[r] = best.col < 0 ? -INFINITY : best.y - l;
}

// one thread per row: the slices' pairs in slice order -> lse; logprobs = logits_at - lse; the targets no tile owns
__global__ __launch_bounds__(256) void readout_score_combine_kernel(const float2* part, int slices, const int32_t* targets, float* logits_at,
                                                                    float* logprobs, float* lse, int64_t R, int K, int64_t V) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float m = -INFINITY, s = 0.f;
    for (int i = 0; i < slices; ++i) {
        const float2 q = part[r * slices + i];
        fold_pair(m, s, q.x, q.y);
    }
    const float l = (m == -INFINITY ? 0.f : m) + logf(s);
    lse[r] = l;
    for (int k = 0; k < K; ++k) {
        const int64_t o = r * K + k;
        const int tg = targets[o];
        float la, lp;
        if (tg == -1) {
            la = 0.f; lp = 0.f;
        } else if (tg < 0 || tg >= V) {
            la = __builtin_nanf(""); lp = la;
        } else {
            la = logits_at[o];
            lp = la - l;
        }
        logits_at[o] = la;
        logprobs[o] = lp;
    }
}

static bool args_in_range(int64_t R, int64_t V) { return R >= 1 && R < (1ll << 31) && V >= 1 && V < (1ll << 31); }

static int auto_slices(int64_t R, int64_t V) {
    const int64_t tiles_m = cdiv64(R, BM), tiles_n = cdiv64(V, BN);
    int64_t s = cdiv64(512, tiles_m);   // 256 CUs x 2 resident workgroups
    if (s > MAX_SLICES) s = MAX_SLICES;
    if (s > tiles_n) s = tiles_n;
    return (int)(s < 1 ? 1 : s);
}

// The draw's split: the number of slices that minimises (rounds of 512 resident workgroups the launch takes) x (tiles in its longest
// slice), the fewest among equals.  The score's choice wherever row tiles x slices comes to 512 (R = 1024: 64, R = 8192: 8); at 150 row
// tiles (R = 19 200) 27 slices — 8 rounds of 19 tiles, 152 against the ideal 150 — where the score's 4 are two rounds of 128, the second
// five sixths empty.  The token does not depend on the split.
static int auto_slices_sample(int64_t R, int64_t V) {
    const int64_t tiles_m = cdiv64(R, BM), tiles_n = cdiv64(V, BN);
    const int64_t most = tiles_n < MAX_SLICES ? tiles_n : MAX_SLICES;
    int64_t best = 1, best_cost = INT64_MAX;
    for (int64_t s = 1; s <= most; ++s) {
        const int64_t cost = cdiv64(tiles_m * s, 512) * cdiv64(tiles_n, s);
        if (cost < best_cost) { best_cost = cost; best = s; }
    }
    return (int)best;
}

}  // namespace obte_score

extern "C" int32_t obte_readout_score_slices(int64_t R, int64_t V) {
    return obte_score::args_in_range(R, V) ? obte_score::auto_slices(R, V) : 1;
}

extern "C" int64_t obte_readout_score_ws_bytes(int64_t R, int64_t V, int32_t slices) {
    if (!obte_score::args_in_range(R, V) || slices < 0 || slices > obte_score::MAX_SLICES) return -1;
    return R * (slices ? slices : obte_score::auto_slices(R, V)) * (int64_t)sizeof(float2);
}

extern "C" int obte_readout_score_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, int64_t R, int64_t V, int64_t C, float alpha,
                                       const void* targets, int64_t K, void* logprobs, void* lse, void* logits_at, int32_t slices, void* ws,
                                       int64_t ws_bytes, obte_stream stream) {
    using namespace obte_score;
    const char* who = "obte_readout_score_bf16";
    OBTE_REQUIRE(x && w && targets && logprobs && lse && logits_at && ws, "%s: null pointer (x, w, targets, logprobs, lse, logits_at, ws)", who);
    OBTE_REQUIRE(R >= 1 && R < (1ll << 31), "%s: R must lie in [1, 2^31), got %lld", who, (long long)R);
    OBTE_REQUIRE(V >= 1 && V < (1ll << 31), "%s: V must lie in [1, 2^31), got %lld", who, (long long)V);
    OBTE_REQUIRE(K >= 1 && K <= MAX_K, "%s: K must lie in [1, %d], got %lld", who, MAX_K, (long long)K);
    OBTE_REQUIRE(C >= BKT && C % BKT == 0, "%s: C must be a positive multiple of 64 (k-contiguous operands), got %lld", who, (long long)C);
    OBTE_REQUIRE(ldx % 8 == 0 && ldx >= C && ldx <= (1ll << 22), "%s: ldx must be a multiple of 8 in [C, 2^22], got %lld", who, (long long)ldx);
    OBTE_REQUIRE(ldw % 8 == 0 && ldw >= C && ldw <= (1ll << 22), "%s: ldw must be a multiple of 8 in [C, 2^22], got %lld", who, (long long)ldw);
    OBTE_REQUIRE(slices >= 0 && slices <= MAX_SLICES, "%s: slices must lie in [0, %d], got %d", who, MAX_SLICES, (int)slices);
    const int64_t need = obte_readout_score_ws_bytes(R, V, slices);
    OBTE_REQUIRE(ws_bytes >= need, "%s: ws_bytes %lld is below the workspace of %lld bytes (obte_readout_score_ws_bytes)", who, (long long)ws_bytes,
                 (long long)need);
    OBTE_REQUIRE_ALIGNED(who, x, "x", 16);
    OBTE_REQUIRE_ALIGNED(who, w, "w", 16);
    OBTE_REQUIRE_ALIGNED(who, ws, "ws", 8);
    OBTE_REQUIRE_ALIGNED(who, targets, "targets", 4);
    OBTE_REQUIRE_ALIGNED(who, logprobs, "logprobs", 4);
    OBTE_REQUIRE_ALIGNED(who, lse, "lse", 4);
    OBTE_REQUIRE_ALIGNED(who, logits_at, "logits_at", 4);

    ScoreParams p;
    p.x = (const bf16*)x; p.w = (const bf16*)w; p.targets = (const int32_t*)targets; p.logits_at = (float*)logits_at; p.part = (float2*)ws;
    p.R = R; p.V = V; p.C = C; p.ldx = ldx; p.ldw = ldw; p.K = K;
    p.x_elems = (R - 1) * ldx + C;   // the operands end with their last row's last element: what follows is not theirs to read
    p.w_elems = (V - 1) * ldw + C;
    p.tiles_m = (int)cdiv64(R, BM); p.tiles_n = (int)cdiv64(V, BN);
    const int want = slices ? slices : auto_slices(R, V);
    p.slices = want < p.tiles_n ? want : p.tiles_n;   // every slice owns at least one tile
    p.alpha = alpha;
    hipStream_t st = (hipStream_t)stream;
    const int rc = gemm_launch<readout_score_kernel, SMEM_BYTES>(p.tiles_m * p.slices, 256, st, p, who);
    if (rc != OBTE_OK) return rc;
    hipLaunchKernelGGL(readout_score_combine_kernel, dim3((unsigned)cdiv64(R, 256)), dim3(256), 0, st, (const float2*)p.part, p.slices, p.targets,
                       p.logits_at, (float*)logprobs, (float*)lse, R, (int)K, V);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}

// ---- the fused draw -------------------------------------------------------------------------------------------------------------------
extern "C" int32_t obte_readout_sample_slices(int64_t R, int64_t V) {
    return obte_score::args_in_range(R, V) ? obte_score::auto_slices_sample(R, V) : 1;
}

extern "C" int64_t obte_readout_sample_ws_bytes(int64_t R, int64_t V, int32_t slices) {
    if (!obte_score::args_in_range(R, V) || slices < 0 || slices > obte_score::MAX_SLICES) return -1;
    return R * (slices ? slices : obte_score::auto_slices_sample(R, V)) * (int64_t)(sizeof(float2) + sizeof(obte_score::Best));
}

extern "C" int obte_readout_sample_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, int64_t R, int64_t V, int64_t C, float alpha, float inv_temp,
                                        uint64_t seed, const int64_t* keys, const void* allowed, int64_t allowed_ld, int32_t* tokens, float* logprob,
                                        float* lse, int32_t slices, void* ws, int64_t ws_bytes, obte_stream stream) {
    using namespace obte_score;
    const char* who = "obte_readout_sample_bf16";
    OBTE_REQUIRE(x && w && tokens && logprob && lse && ws, "%s: null pointer (x, w, tokens, logprob, lse, ws)", who);
    OBTE_REQUIRE(R >= 1 && R < (1ll << 31), "%s: R must lie in [1, 2^31), got %lld", who, (long long)R);
    OBTE_REQUIRE(V >= 1 && V < (1ll << 31), "%s: V must lie in [1, 2^31), got %lld", who, (long long)V);
    OBTE_REQUIRE(C >= BKT && C % BKT == 0, "%s: C must be a positive multiple of 64 (k-contiguous operands), got %lld", who, (long long)C);
    OBTE_REQUIRE(ldx % 8 == 0 && ldx >= C && ldx <= (1ll << 22), "%s: ldx must be a multiple of 8 in [C, 2^22], got %lld", who, (long long)ldx);
    OBTE_REQUIRE(ldw % 8 == 0 && ldw >= C && ldw <= (1ll << 22), "%s: ldw must be a multiple of 8 in [C, 2^22], got %lld", who, (long long)ldw);
    OBTE_REQUIRE(inv_temp >= 0.f && inv_temp <= 3.4028234e38f, "%s: inv_temp must be finite and not negative, got %g", who, (double)inv_temp);
    OBTE_REQUIRE(allowed_ld >= 0, "%s: allowed_ld must not be negative, got %lld", who, (long long)allowed_ld);
    OBTE_REQUIRE(allowed_ld == 0 || allowed_ld >= (V + 7) / 8, "%s: allowed_ld %lld is smaller than the ceil(V / 8) = %lld bytes of a mask row", who,
                 (long long)allowed_ld, (long long)((V + 7) / 8));
    OBTE_REQUIRE(slices >= 0 && slices <= MAX_SLICES, "%s: slices must lie in [0, %d], got %d", who, MAX_SLICES, (int)slices);
    const int64_t need = obte_readout_sample_ws_bytes(R, V, slices);
    OBTE_REQUIRE(ws_bytes >= need, "%s: ws_bytes %lld is below the workspace of %lld bytes (obte_readout_sample_ws_bytes)", who, (long long)ws_bytes,
                 (long long)need);
    OBTE_REQUIRE_ALIGNED(who, x, "x", 16);
    OBTE_REQUIRE_ALIGNED(who, w, "w", 16);
    OBTE_REQUIRE_ALIGNED(who, ws, "ws", 8);
    OBTE_REQUIRE_ALIGNED(who, keys, "keys", 8);
    OBTE_REQUIRE_ALIGNED(who, tokens, "tokens", 4);
    OBTE_REQUIRE_ALIGNED(who, logprob, "logprob", 4);
    OBTE_REQUIRE_ALIGNED(who, lse, "lse", 4);

    SampleParams p;
    p.x = (const bf16*)x; p.w = (const bf16*)w; p.keys = keys; p.allowed = (const uint8_t*)allowed;
    p.R = R; p.V = V; p.C = C; p.ldx = ldx; p.ldw = ldw; p.allowed_ld = allowed_ld;
    p.x_elems = (R - 1) * ldx + C;
    p.w_elems = (V - 1) * ldw + C;
    p.tiles_m = (int)cdiv64(R, BM); p.tiles_n = (int)cdiv64(V, BN);
    const int want = slices ? slices : auto_slices_sample(R, V);
    p.slices = want < p.tiles_n ? want : p.tiles_n;
    p.part = (float2*)ws;
    p.best = (Best*)((char*)ws + R * p.slices * (int64_t)sizeof(float2));   // behind the pairs: 4-byte members
    p.alpha = alpha;
    p.greedy = inv_temp == 0.f;
    p.inv_temp = p.greedy ? 1.f : inv_temp;
    p.noise = make_drop(0.f, seed, OBTE_SITE_FILL);
    hipStream_t st = (hipStream_t)stream;
    const int rc = gemm_launch<readout_sample_kernel, SMEM_BYTES>(p.tiles_m * p.slices, 256, st, p, who);
    if (rc != OBTE_OK) return rc;
    hipLaunchKernelGGL(readout_sample_combine_kernel, dim3((unsigned)cdiv64(R, 256)), dim3(256), 0, st, (const float2*)p.part, (const Best*)p.best, p.slices,
                       tokens, logprob, lse, R);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}

// ---- the unmasking loop's bookkeeping ------------------------------------------------------------------------------------------------------
namespace obte_fill {

constexpr int MAX_SEG = 8192, THREADS = 256, PER = MAX_SEG / THREADS;

struct CommitParams {
    const int64_t* rows; const int32_t* seg_off; const int32_t* tokens; const float* logprob; const int32_t* take;
    int64_t* idx; float* out_logprob; int64_t* rows_next; const int32_t* seg_off_next;
    int64_t n, n_idx, n_next;
    int32_t max_seg, order;
    DropCfg cfg;
};

// One workgroup per sequence.  Every entry gets a 32-bit sort word (smaller = earlier) in LDS; an entry's rank is the number of entries
// whose (word, index) is smaller — counted by its own thread, n_b^2 comparisons per sequence in all — and it is selected when its rank
// is below take.  Thread t then owns the contiguous entries [t per, (t + 1) per): a scan of the threads' counts of entries left over
// gives each its place in rows_next, ascending as the entries are.
__global__ __launch_bounds__(THREADS) void fill_commit_kernel(CommitParams a) {
    __shared__ uint32_t word[MAX_SEG];
    __shared__ uint8_t sel[MAX_SEG];
    __shared__ int32_t left_before[THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const int64_t lo = a.seg_off[b], hi = a.seg_off[b + 1];
    if (lo < 0 || hi < lo || hi > a.n || hi - lo > a.max_seg) return;   // (uniform over the workgroup)
    const int nb = (int)(hi - lo);
    const int tk = a.take[b];
    const int take = tk < 0 || tk > nb ? 0 : tk;
    const int64_t o_lo = a.seg_off_next[b], o_hi0 = a.seg_off_next[b + 1];
    const int64_t o_hi = o_hi0 < a.n_next ? o_hi0 : a.n_next;

    for (int i = t; i < nb; i += THREADS) {
        uint32_t k = 0;                                             // OBTE_FILL_LEFT: the index alone decides
        if (a.order == OBTE_FILL_CONFIDENCE) {
            float lp = a.logprob[lo + i];
            if (!(lp == lp)) lp = -INFINITY;
            if (lp == 0.f) lp = 0.f;                                // -0 ranks as +0
            const uint32_t u = __float_as_uint(lp);
            k = ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));      // ascending in the float, then reversed: the larger logprob first
        } else if (a.order == OBTE_FILL_RANDOM) {
            k = drop_rowkey((uint64_t)a.rows[lo + i], a.cfg);
        }
        word[i] = k;
    }
    __syncthreads();
    for (int i = t; i < nb; i += THREADS) {
        const uint32_t k = word[i];
        int rank = 0;
        for (int j = 0; j < nb; ++j) {
            const uint32_t kj = word[j];
            rank += (kj < k || (kj == k && j < i)) ? 1 : 0;
        }
        sel[i] = rank < take;
    }
    __syncthreads();
    const int per = (nb + THREADS - 1) / THREADS;
    const int i0 = t * per < nb ? t * per : nb, i1 = i0 + per < nb ? i0 + per : nb;
    int mine = 0;
    for (int i = i0; i < i1; ++i) mine += sel[i] ? 0 : 1;
    left_before[t] = mine;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {                        // inclusive scan
        const int add = t >= d ? left_before[t - d] : 0;
        __syncthreads();
        left_before[t] += add;
        __syncthreads();
    }
    int64_t o = o_lo + left_before[t] - mine;
    for (int i = i0; i < i1; ++i) {
        const int64_t pos = a.rows[lo + i];
        if (sel[i]) {
            if (pos >= 0 && pos < a.n_idx) {
                a.idx[pos] = a.tokens[lo + i];
                a.out_logprob[pos] = a.logprob[lo + i];
            }
        } else {
            if (o >= 0 && o >= o_lo && o < o_hi) a.rows_next[o] = pos;
            ++o;
        }
    }
}

}  // namespace obte_fill

extern "C" int obte_fill_commit(const int64_t* rows, const int32_t* seg_off, int64_t n, int64_t B, int32_t max_seg, const int32_t* tokens,
                                const float* logprob, const int32_t* take, int32_t order, uint64_t seed, int64_t* idx, float* out_logprob, int64_t n_idx,
                                int64_t* rows_next, const int32_t* seg_off_next, int64_t n_next, obte_stream stream) {
    using namespace obte_fill;
    const char* who = "obte_fill_commit";
    OBTE_REQUIRE(rows && seg_off && tokens && logprob && take && idx && out_logprob && rows_next && seg_off_next,
                 "%s: null pointer (rows, seg_off, tokens, logprob, take, idx, out_logprob, rows_next, seg_off_next)", who);
    OBTE_REQUIRE(B >= 1 && B < (1ll << 31), "%s: B must lie in [1, 2^31), got %lld", who, (long long)B);
    OBTE_REQUIRE(n >= 0 && n_next >= 0, "%s: n and n_next must not be negative, got %lld and %lld", who, (long long)n, (long long)n_next);
    OBTE_REQUIRE(n_idx >= 1, "%s: n_idx must be at least 1, got %lld", who, (long long)n_idx);
    OBTE_REQUIRE(max_seg >= 0 && max_seg <= MAX_SEG, "%s: max_seg must lie in [0, %d] (entries per sequence), got %d", who, MAX_SEG, (int)max_seg);
    OBTE_REQUIRE(order == OBTE_FILL_CONFIDENCE || order == OBTE_FILL_RANDOM || order == OBTE_FILL_LEFT, "%s: order must be 0 (confidence), 1 (random) or "
                 "2 (left), got %d", who, (int)order);
    OBTE_REQUIRE((const void*)rows != (const void*)rows_next, "%s: rows_next must not be rows", who);
    OBTE_REQUIRE_ALIGNED(who, rows, "rows", 8);
    OBTE_REQUIRE_ALIGNED(who, rows_next, "rows_next", 8);
    OBTE_REQUIRE_ALIGNED(who, idx, "idx", 8);
    OBTE_REQUIRE_ALIGNED(who, seg_off, "seg_off", 4);
    OBTE_REQUIRE_ALIGNED(who, seg_off_next, "seg_off_next", 4);
    OBTE_REQUIRE_ALIGNED(who, tokens, "tokens", 4);
    OBTE_REQUIRE_ALIGNED(who, logprob, "logprob", 4);
    OBTE_REQUIRE_ALIGNED(who, take, "take", 4);
    OBTE_REQUIRE_ALIGNED(who, out_logprob, "out_logprob", 4);
    CommitParams a;
    a.rows = rows; a.seg_off = seg_off; a.tokens = tokens; a.logprob = logprob; a.take = take; a.idx = idx; a.out_logprob = out_logprob;
    a.rows_next = rows_next; a.seg_off_next = seg_off_next; a.n = n; a.n_idx = n_idx; a.n_next = n_next; a.max_seg = max_seg; a.order = order;
    a.cfg = make_drop(0.f, seed, OBTE_SITE_FILL);
    hipLaunchKernelGGL(fill_commit_kernel, dim3((unsigned)B), dim3(THREADS), 0, (hipStream_t)stream, a);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}
