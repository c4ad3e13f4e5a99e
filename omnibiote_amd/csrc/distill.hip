// Distillation loss over listed rows (include/omnibiote_hip_distill.h): cross entropy against the labels plus the temperature-scaled
// KL(teacher || student), loss and d(logits) in one launch.  The CE family of elementwise.hip with a second operand row.
#include "common.h"
#include "../../include/omnibiote_hip_distill.h"
#include <math.h>

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kThreads = 512;   // see the register budget below

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }   // v_exp_f32; every argument here is <= 0

// One workgroup per row.  Register budget: masked_ce_regs_kernel<32> keeps ONE 65 536-wide row in 128 VGPRs per thread at 256 threads;
// two rows at 256 threads would be 256 VGPRs of operands alone.  512 threads halve the share of each thread: NCH = 16 chunks of 8
// elements per row, 64 + 64 VGPRs for the two rows, and the workgroup's 8 waves (two per SIMD) may each use up to 256 registers, so
// the reductions and the gradient pass fit beside the operands without scratch.  The other choice, 256 threads and half a row per
// pass, would read both rows twice.  NCH = 0: the streamed form for wider rows — the same chunks in the same order per thread, read
// from memory in both passes (the second read comes from L2), so its results are bitwise those of a register form of that width.
// Three (max, sum) pairs per row — of s, b s and b t; the first two share their maximum (b > 0) and coincide at b = 1 (BETA1) — and
// the teacher-weighted sum of (t - s) that rides on the third.
template <int NCH, bool BETA1>
__global__ __launch_bounds__(kThreads) void distill_ce_kernel(const bf16* __restrict__ logits, const bf16* __restrict__ teacher,
                                                              const int64_t* __restrict__ target, float row_scale,
                                                              const float* __restrict__ row_scale_vec, float ce_weight, float kl_weight, float beta,
                                                              float* __restrict__ row_loss, float* __restrict__ row_ce, float* __restrict__ row_kl,
                                                              bf16* __restrict__ dlogits, int64_t vocab64) {
    __shared__ float red[8][8];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int vocab = (int)vocab64;   // <= 131 072: 32-bit offsets from the row's (uniform) base
    const bf16* srow = logits + r * vocab64;
    const bf16* trow = teacher + r * vocab64;
    bf16* drow = dlogits + r * vocab64;
    const int toff = tid * 8;
    const int mine = (vocab / 8 - tid + kThreads - 1) / kThreads;   // the thread's chunks: c = (i * kThreads + tid) * 8 < vocab for i < mine
    constexpr int NR = NCH > 0 ? NCH : 1;
    bf16x8 vs[NR], vt[NR];
    if constexpr (NCH > 0) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            vs[i] = bf16x8{};
            vt[i] = bf16x8{};
            if (i < mine) {   // chunk i: a uniform base per chunk plus the thread's own 16 bytes
                vs[i] = *reinterpret_cast<const bf16x8*>(srow + i * (kThreads * 8) + toff);
                vt[i] = *reinterpret_cast<const bf16x8*>(trow + i * (kThreads * 8) + toff);
            }
        }
    }
    const float kb = beta * kLog2e;
    // pass 1: online max / sums per thread
    float ms = -INFINITY, ls = 0.f, lbs = 0.f, mt = -INFINITY, lbt = 0.f, a = 0.f;
    auto reduce_chunk = [&](const bf16x8& xs, const bf16x8& xt) {
        float s[8], t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { s[j] = bf2f(xs[j]); t[j] = bf2f(xt[j]); }
        float mxs = s[0], mxt = t[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) { mxs = fmaxf(mxs, s[j]); mxt = fmaxf(mxt, t[j]); }
        const float ns = fmaxf(ms, mxs), nt = fmaxf(mt, mxt);
        const float os = -ns * kLog2e, obs = -ns * kb, obt = -nt * kb;
        float adds = 0.f, addbs = 0.f, addbt = 0.f, adda = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            adds += ex2(__builtin_fmaf(s[j], kLog2e, os));              // exp(s - max): one FMA, one v_exp
            if (!BETA1) addbs += ex2(__builtin_fmaf(s[j], kb, obs));    // exp(b (s - max))
            const float e = ex2(__builtin_fmaf(t[j], kb, obt));         // exp(b (t - max))
            addbt += e;
            adda += e * (t[j] - s[j]);
        }
        ls = ls * ex2((ms - ns) * kLog2e) + adds;
        if (!BETA1) lbs = lbs * ex2((ms - ns) * kb) + addbs;
        const float ft = ex2((mt - nt) * kb);
        lbt = lbt * ft + addbt;
        a = a * ft + adda;
        ms = ns;
        mt = nt;
    };
    if constexpr (NCH > 0) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            if (i < mine) reduce_chunk(vs[i], vt[i]);
            __builtin_amdgcn_sched_barrier(0);   // chunk by chunk: left to itself hipcc converts the whole row to fp32 first and spills
        }
    } else {
        for (int i = 0; i < mine; ++i)
            reduce_chunk(*reinterpret_cast<const bf16x8*>(srow + i * (kThreads * 8) + toff), *reinterpret_cast<const bf16x8*>(trow + i * (kThreads * 8) + toff));
    }
    // per wave, then through LDS (threads, or whole waves, without elements hold -inf and contribute zeros)
    const float wms = wave_max(ms), wmt = wave_max(mt);
    const bool has_s = ms != -INFINITY, has_t = mt != -INFINITY;
    ls = wave_sum(has_s ? ls * ex2((ms - wms) * kLog2e) : 0.f);
    if (!BETA1) lbs = wave_sum(has_s ? lbs * ex2((ms - wms) * kb) : 0.f);
    const float ftw = has_t ? ex2((mt - wmt) * kb) : 0.f;
    lbt = wave_sum(lbt * ftw);
    a = wave_sum(a * ftw);
    if (lane == 0) {
        red[wave][0] = wms; red[wave][1] = ls; red[wave][2] = lbs;
        red[wave][3] = wmt; red[wave][4] = lbt; red[wave][5] = a;
    }
    __syncthreads();
    float bms = red[0][0], bmt = red[0][3];
#pragma unroll
    for (int w = 1; w < 8; ++w) { bms = fmaxf(bms, red[w][0]); bmt = fmaxf(bmt, red[w][3]); }
    float bls = 0.f, blbs = 0.f, blbt = 0.f, ba = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        const bool ws_ = red[w][0] != -INFINITY, wt_ = red[w][3] != -INFINITY;
        bls += ws_ ? red[w][1] * ex2((red[w][0] - bms) * kLog2e) : 0.f;
        if (!BETA1) blbs += ws_ ? red[w][2] * ex2((red[w][0] - bms) * kb) : 0.f;
        const float f = wt_ ? ex2((red[w][3] - bmt) * kb) : 0.f;
        blbt += red[w][4] * f;
        ba += red[w][5] * f;
    }
    const float lse_s = bms + logf(bls);
    const float lse_bs = BETA1 ? lse_s : beta * bms + logf(blbs);
    const float lse_bt = beta * bmt + logf(blbt);
    const int64_t tgt64 = target[r];
    const int tgt = tgt64 < 0 ? 0 : (tgt64 >= vocab ? vocab - 1 : (int)tgt64);
    const float w = row_scale_vec ? row_scale * row_scale_vec[r] : row_scale;
    if (tid == 0) {
        const float ce = lse_s - bf2f(srow[tgt]);
        const float kl = beta * ba / blbt + (lse_bs - lse_bt);
        row_loss[r] = w * (ce_weight * ce + kl_weight * kl);
        if (row_ce) row_ce[r] = ce;
        if (row_kl) row_kl[r] = kl;
    }
    // pass 2: the gradient, out of the registers (or the second read)
    const float a1 = w * ce_weight, a2 = w * kl_weight * beta;
    const float cs = -lse_s * kLog2e, cbs = -lse_bs * kLog2e, cbt = -lse_bt * kLog2e;
    auto grad_chunk = [&](const bf16x8& xs, const bf16x8& xt, int base) {   // base: the chunk's first column of thread 0
        const int tj = tgt - base - toff;   // the target's place in this thread's 8 columns, if it is one of them
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float sj = bf2f(xs[j]);
            float P = ex2(__builtin_fmaf(sj, kLog2e, cs));
            const float p = BETA1 ? P : ex2(__builtin_fmaf(sj, kb, cbs));
            const float q = ex2(__builtin_fmaf(bf2f(xt[j]), kb, cbt));
            if (j == tj) P -= 1.0f;
            o[j] = f2bf(a1 * P + a2 * (p - q));
        }
        *reinterpret_cast<bf16x8*>(drow + base + toff) = o;
    };
    if constexpr (NCH > 0) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            // (the operands pass through an empty asm: otherwise hipcc keeps pass 1's fp32 conversions of the whole row for this pass and spills them)
            asm volatile("" : "+v"(vs[i]), "+v"(vt[i]));
            if (i < mine) grad_chunk(vs[i], vt[i], i * (kThreads * 8));
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        for (int i = 0; i < mine; ++i)
            grad_chunk(*reinterpret_cast<const bf16x8*>(srow + i * (kThreads * 8) + toff), *reinterpret_cast<const bf16x8*>(trow + i * (kThreads * 8) + toff),
                       i * (kThreads * 8));
    }
}

template <int NCH>
void launch(bool beta1, dim3 grid, hipStream_t st, const bf16* logits, const bf16* teacher, const int64_t* target, float row_scale,
            const float* row_scale_vec, float ce_weight, float kl_weight, float beta, float* row_loss, float* row_ce, float* row_kl, bf16* dlogits,
            int64_t vocab) {
    if (beta1)
        hipLaunchKernelGGL((distill_ce_kernel<NCH, true>), grid, dim3(kThreads), 0, st, logits, teacher, target, row_scale, row_scale_vec, ce_weight,
                           kl_weight, beta, row_loss, row_ce, row_kl, dlogits, vocab);
    else
        hipLaunchKernelGGL((distill_ce_kernel<NCH, false>), grid, dim3(kThreads), 0, st, logits, teacher, target, row_scale, row_scale_vec, ce_weight,
                           kl_weight, beta, row_loss, row_ce, row_kl, dlogits, vocab);
}

bool overlaps(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

}   // namespace

extern "C" int obte_distill_ce_rows(const obte_bf16* logits, const obte_bf16* teacher_logits, const int64_t* target,
                                    float row_scale, const float* row_scale_vec, float ce_weight, float kl_weight, float inv_temperature,
                                    float* row_loss, float* row_ce, float* row_kl, obte_bf16* dlogits, int64_t n_rows, int64_t vocab,
                                    obte_stream s) {
    OBTE_REQUIRE(logits && teacher_logits && target && row_loss && dlogits, "obte_distill_ce_rows: null pointer");
    OBTE_REQUIRE_ALIGNED("obte_distill_ce_rows", logits, "logits", 16);
    OBTE_REQUIRE_ALIGNED("obte_distill_ce_rows", teacher_logits, "teacher_logits", 16);
    OBTE_REQUIRE_ALIGNED("obte_distill_ce_rows", dlogits, "dlogits", 16);
    OBTE_REQUIRE(n_rows > 0 && n_rows < (1ll << 31), "obte_distill_ce_rows: need 0 < n_rows < 2^31, got %lld", (long long)n_rows);
    OBTE_REQUIRE(vocab >= 8 && vocab % 8 == 0 && vocab <= 131072, "obte_distill_ce_rows: vocab must be a multiple of 8 in [8, 131072], got %lld",
                 (long long)vocab);
    OBTE_REQUIRE(isfinite(inv_temperature) && inv_temperature > 0.f, "obte_distill_ce_rows: inv_temperature must be a positive finite number");
    OBTE_REQUIRE(isfinite(row_scale) && isfinite(ce_weight) && isfinite(kl_weight), "obte_distill_ce_rows: row_scale, ce_weight and kl_weight must be finite");
    const size_t bytes = (size_t)n_rows * (size_t)vocab * 2;
    OBTE_REQUIRE(!overlaps(dlogits, logits, bytes) && !overlaps(dlogits, teacher_logits, bytes),
                 "obte_distill_ce_rows: dlogits must not alias logits or teacher_logits");
    const dim3 grid((unsigned)n_rows);
    const bool beta1 = inv_temperature == 1.0f;
    const bf16* lg = (const bf16*)logits;
    const bf16* tl = (const bf16*)teacher_logits;
    if (vocab <= kThreads * 4 * 8)
        launch<4>(beta1, grid, (hipStream_t)s, lg, tl, target, row_scale, row_scale_vec, ce_weight, kl_weight, inv_temperature, row_loss, row_ce, row_kl,
                  (bf16*)dlogits, vocab);
    else if (vocab <= kThreads * 16 * 8)
        launch<16>(beta1, grid, (hipStream_t)s, lg, tl, target, row_scale, row_scale_vec, ce_weight, kl_weight, inv_temperature, row_loss, row_ce, row_kl,
                   (bf16*)dlogits, vocab);
    else
        launch<0>(beta1, grid, (hipStream_t)s, lg, tl, target, row_scale, row_scale_vec, ce_weight, kl_weight, inv_temperature, row_loss, row_ce, row_kl,
                  (bf16*)dlogits, vocab);
    OBTE_CHECK_LAUNCH("obte_distill_ce_rows");
    return OBTE_OK;
}
