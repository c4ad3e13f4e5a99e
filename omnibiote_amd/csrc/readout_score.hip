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
#include <math.h>
#include "gemm_common.h"
#include "../../include/omnibiote_hip_score.h"

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
    const bf16* x; const bf16* w; const int32_t* targets; float* logits_at; float2* part;
    int64_t R, V, C, ldx, ldw, K;
    int64_t x_elems, w_elems;
    int tiles_m, tiles_n, slices;
    float alpha;
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

__device__ __forceinline__ float exp2_of(float d) { return __builtin_amdgcn_exp2f(d * LOG2E); }   // e^d; d = -inf gives 0

// (m, s) <- (m, s) and (m2, s2), in that order; s counts in units of e^m.  No inf - inf: an all -inf side scales by e^(-inf - 0) = 0.
__device__ __forceinline__ void fold_pair(float& m, float& s, float m2, float s2) {
    const float mx = fmaxf(m, m2);
    const float ms = mx == -INFINITY ? 0.f : mx;
    s = s * exp2_of(m - ms) + s2 * exp2_of(m2 - ms);
    m = mx;
}

__global__ __launch_bounds__(256, 2) void readout_score_kernel(ScoreParams p) {
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
    const int K = (int)p.K;
    const char* my_rows = smem + (srow >> 6) * 2 * EPI_WAVE_BYTES + (srow & 63) * EPI_LD;   // + (column >> 6) * EPI_WAVE_BYTES + (column & 63) * 2
    float run_m = -INFINITY, run_s = 0.f, run_c = 0.f;   // the row half's maximum, the sum of e^(z - maximum), what the sum's additions lost
    const int tg0 = row_ok && shalf < K ? p.targets[grow * K + shalf] : -1;   // targets k = shalf, shalf + 2, ...: the first stays in a register

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
        if (lim == 64) {
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
        if (lim == 64) {
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
        const float f = exp2_of(run_m - ms);   // 1 unless the maximum moved
        const float s_old = run_s * f;
        const float s_new = s_old + tsum;
        run_c = run_c * f + (s_old >= tsum ? (s_old - s_new) + tsum : (tsum - s_new) + s_old);
        run_s = s_new;
        run_m = mnew;

        // ---- targets of this row that lie in this tile --------------------------------------------------------------------------------
        if (row_ok) {
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
    float m = shalf ? om : run_m, s = shalf ? os : mine;
    fold_pair(m, s, shalf ? run_m : om, shalf ? mine : os);
    if (row_ok && shalf == 0) p.part[grow * p.slices + sl] = make_float2(m, s);
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
