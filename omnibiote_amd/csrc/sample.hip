// Next-token sampling on the device (include/omnibiote_hip_sample.h): temperature, top-k, top-p, softmax and the draw, one workgroup
// per row of bf16 logits, the row read once and held in registers as order-preserving 16-bit keys for every pass (sample_common.h:
// the load, the maximum, the select and the weights).
//   draw     per-wave integer totals -> the wave that holds floor(u total); there one wave scan per register group finds the lane,
//            and the lane walks its 8 columns.
// CON: the restricted form (include/omnibiote_hip_constrain.h) — the load clears the excluded keys, everything after it is the same code.
// PEN: the penalised form (include/omnibiote_hip_penalty.h), built on the restricted load — the load also rewrites the columns of the
// row's history from a table in dynamic LDS; the select's histogram then takes the table's place, so V = 65536 fits the 160 KiB.
#include "sample_common.h"
#include <type_traits>

namespace {

struct SampleParams {
    const bf16* logits;
    int64_t ld;
    const float* u;
    int64_t* token;
    int32_t* n_kept;
    float scale;      // log2(e) / temperature
    float top_p;
    int32_t V, top_k, greedy;
    SpConstraint con;   // read by the CON kernels only
};
struct SamplePenParams : SampleParams {
    SpPenalty pen;
};
extern __shared__ __align__(16) unsigned char sp_dyn[];   // PEN: max(16 ceil(V / 8), 8 SP_BINS) bytes, the history table, then hist

template <int NT, int R, bool CON, bool PEN = false>
__global__ __launch_bounds__(NT) void sample_kernel(std::conditional_t<PEN, SamplePenParams, SampleParams> p) {
    u64* hist;
    if constexpr (PEN) {
        hist = reinterpret_cast<u64*>(sp_dyn);
    } else {
        __shared__ u64 hist_s[SP_BINS];
        hist = hist_s;
    }
    __shared__ u64 hist2[16];
    __shared__ u64 red[NT / 64];
    __shared__ u64 red_n[NT / 64];
    __shared__ u64 sel[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x;
    const bf16* x = p.logits + row * p.ld;
    const int V = p.V;
    const int chunk0 = wave * R * 64 + lane;

    uint32_t k[R][4];
    if constexpr (PEN) sp_load_row_penalized<NT, R>(x, chunk0, V, sp_row_mask(p.con, row, 0), p.pen, row, reinterpret_cast<uint32_t*>(sp_dyn), k);
    else if (CON) sp_load_row_masked<R>(x, chunk0, V, sp_row_mask(p.con, row, 0), k);
    else sp_load_row<R>(x, chunk0, V, k);
    const uint32_t best = sp_row_max<NT, R>(k, chunk0, red);
    const uint32_t maxkey = best >> 16;
    const int argmax = 65535 - (int)(best & 0xFFFFu);
    if (maxkey == 0 || p.greedy) {   // nothing to sample: token 0, nothing kept
        if (tid == 0) {
            p.token[row] = maxkey ? argmax : 0;
            if (p.n_kept) p.n_kept[row] = maxkey ? 1 : 0;
        }
        return;
    }
    const float maxv = sp_val(maxkey), scale = p.scale;
    const uint32_t thr = sp_threshold<NT, R>(k, maxkey, maxv, scale, V, p.top_k, p.top_p, hist, hist2, red, sel);

    // the draw
    u64 mass, base, total, n;
    sp_row_mass<NT, R>(k, thr, maxkey, maxv, scale, red, red_n, mass, base, total, n);
    if (tid == 0 && p.n_kept) p.n_kept[row] = (int32_t)n;
    const u64 target = sp_draw_target(p.u[row], total);
    if (!(base <= target && target < base + mass)) return;   // (mass: the wave's total after the reduction) one wave goes on

    u64 run = base;
    bool found = false;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (found) break;
        const int c = chunk0 + j * 64;
        u64 sj = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t a = k[j][q] & 0xFFFFu, b = k[j][q] >> 16;
            sj += a >= thr ? sp_weight(a, maxkey, maxv, scale) : 0ull;
            sj += b >= thr ? sp_weight(b, maxkey, maxv, scale) : 0ull;
        }
        const u64 inc = sp_wave_scan(sj);
        const u64 tot = __shfl(inc, 63, 64);
        if (target < run + tot) {
            found = true;
            const u64 hit = __ballot(run + inc > target);
            if (lane == __ffsll((long long)hit) - 1) {
                u64 cum = run + inc - sj;
                int tok = -1;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t a = k[j][q] & 0xFFFFu, b = k[j][q] >> 16;
                    cum += a >= thr ? sp_weight(a, maxkey, maxv, scale) : 0ull;
                    if (tok < 0 && cum > target) tok = c * 8 + 2 * q;
                    cum += b >= thr ? sp_weight(b, maxkey, maxv, scale) : 0ull;
                    if (tok < 0 && cum > target) tok = c * 8 + 2 * q + 1;
                }
                p.token[row] = tok < 0 ? argmax : tok;
            }
        }
        run += tot;
    }
}

// the host's checks of a call's penalties (OBTE_EINVAL before any launch); `changes`: whether any column of any row can come out different
int sp_check_penalty(const char* who, const SpPenalty& q, bool* changes) {
    OBTE_REQUIRE(q.prompt_max >= 0 && q.gen_max >= 0, "%s: prompt_max and gen_max must not be negative, got %d and %d", who, (int)q.prompt_max, (int)q.gen_max);
    OBTE_REQUIRE(q.gen_max <= 32767, "%s: gen_max = %d exceeds the 32767 a column's count holds", who, (int)q.gen_max);
    OBTE_REQUIRE(q.gen_max <= q.gen_ld, "%s: gen_max %d is larger than gen_ld %lld", who, (int)q.gen_max, (long long)q.gen_ld);
    OBTE_REQUIRE(q.prompt_max < (1 << 24), "%s: prompt_max = %d must lie below 2^24", who, (int)q.prompt_max);
    OBTE_REQUIRE(q.prompt_max <= q.prompt_ld, "%s: prompt_max %d is larger than prompt_ld %lld", who, (int)q.prompt_max, (long long)q.prompt_ld);
    OBTE_REQUIRE(q.prompt || q.prompt_max == 0, "%s: null pointer (prompt) with prompt_max = %d", who, (int)q.prompt_max);
    OBTE_REQUIRE(q.gen || q.gen_max == 0, "%s: null pointer (gen) with gen_max = %d", who, (int)q.gen_max);
    OBTE_REQUIRE_ALIGNED(who, q.prompt, "prompt", 8);
    OBTE_REQUIRE_ALIGNED(who, q.gen, "gen", 8);
    OBTE_REQUIRE_ALIGNED(who, q.prompt_len, "prompt_len", 4);
    OBTE_REQUIRE_ALIGNED(who, q.n_gen, "n_gen", 4);
    OBTE_REQUIRE(isfinite(q.repetition) && isfinite(q.inv_repetition) && isfinite(q.presence) && isfinite(q.frequency),
                 "%s: repetition, inv_repetition, presence and frequency must be finite", who);
    OBTE_REQUIRE(q.repetition > 0.f, "%s: repetition must be positive", who);
    *changes = (q.prompt_max > 0 || q.gen_max > 0) && !(q.repetition == 1.f && q.presence == 0.f && q.frequency == 0.f);
    return OBTE_OK;
}

// the PEN kernel with its dynamic LDS: the table of this V's columns, and no less than the histogram that follows it there
template <int NT, int R>
void sample_launch_penalized(int64_t B, int64_t V, hipStream_t st, const SamplePenParams& p) {
    constexpr int MAX_BYTES = NT * R * 16 > SP_BINS * 8 ? NT * R * 16 : SP_BINS * 8;
    static const hipError_t attr = hipFuncSetAttribute((const void*)sample_kernel<NT, R, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_BYTES);
    (void)attr;
    const int table = (int)((V + 7) / 8) * 16;
    hipLaunchKernelGGL((sample_kernel<NT, R, true, true>), dim3((unsigned)B), dim3(NT), table > SP_BINS * 8 ? table : SP_BINS * 8, st, p);
}

// the three entry points: `con` NULL is obte_sample_logits_bf16 itself; `pen` (with `con`): obte_sample_logits_penalized_bf16, which
// takes the restricted kernels when its penalties change nothing
int sample_launch(const char* who, const obte_bf16* logits, int64_t ld, int64_t B, int64_t V, const float* u, float temperature, int32_t top_k, float top_p,
                  const SpConstraint* con, int64_t hold_token, int64_t* token, int32_t* n_kept, obte_stream s, const SpPenalty* pen = nullptr) {
    OBTE_REQUIRE(logits && token, "%s: null pointer (logits, token)", who);
    OBTE_REQUIRE(B >= 1 && B < (1ll << 31) && V >= 1, "%s: B and V must be at least 1 (B=%lld V=%lld)", who, (long long)B, (long long)V);
    if (V > SP_MAX_V) {
        obte_set_error("%s: V = %lld exceeds the %d columns a workgroup holds in registers", who, (long long)V, SP_MAX_V);
        return OBTE_EUNSUPPORTED;
    }
    OBTE_REQUIRE(ld % 8 == 0, "%s: ld must be a multiple of 8 (16-byte rows), got %lld", who, (long long)ld);
    OBTE_REQUIRE(ld >= V, "%s: ld %lld is smaller than V %lld", who, (long long)ld, (long long)V);
    OBTE_REQUIRE_ALIGNED(who, logits, "logits", 16);
    OBTE_REQUIRE(temperature >= 0.f && isfinite(temperature), "%s: temperature must be finite and not negative", who);
    OBTE_REQUIRE(top_p > 0.f && top_p <= 1.f, "%s: top_p must lie in (0, 1]", who);
    OBTE_REQUIRE_ALIGNED(who, u, "u", 4);
    OBTE_REQUIRE_ALIGNED(who, n_kept, "n_kept", 4);
    OBTE_REQUIRE_ALIGNED(who, token, "token", 8);
    SamplePenParams pp;
    SampleParams& p = pp;
    p.logits = (const bf16*)logits; p.ld = ld; p.u = u; p.token = token; p.n_kept = n_kept;
    p.V = (int32_t)V; p.top_k = top_k; p.top_p = top_p;
    p.greedy = (!u || temperature == 0.f || top_k == 1) ? 1 : 0;
    p.scale = p.greedy ? 1.f : (float)(1.4426950408889634 / (double)temperature);
    p.con = SpConstraint{nullptr, 0, nullptr, -1, 0};
    if (con) {
        const int rc = sp_check_constraint(who, *con, hold_token, V, &p.con);
        if (rc != OBTE_OK) return rc;
    }
    bool penalized = false;
    if (pen) {
        const int rc = sp_check_penalty(who, *pen, &penalized);
        if (rc != OBTE_OK) return rc;
        pp.pen = *pen;
    }
    hipStream_t st = (hipStream_t)s;
    const int prof = obte_prof_begin(st, 114, B, V, p.greedy);
    const dim3 grid((unsigned)B);
    if (penalized) {
        if (V <= 256 * 8) sample_launch_penalized<256, 1>(B, V, st, pp);
        else if (V <= 1024 * 8 * 2) sample_launch_penalized<1024, 2>(B, V, st, pp);
        else sample_launch_penalized<1024, 8>(B, V, st, pp);
    } else if (con) {
        if (V <= 256 * 8) hipLaunchKernelGGL((sample_kernel<256, 1, true>), grid, dim3(256), 0, st, p);
        else if (V <= 1024 * 8 * 2) hipLaunchKernelGGL((sample_kernel<1024, 2, true>), grid, dim3(1024), 0, st, p);
        else hipLaunchKernelGGL((sample_kernel<1024, 8, true>), grid, dim3(1024), 0, st, p);
    } else {
        if (V <= 256 * 8) hipLaunchKernelGGL((sample_kernel<256, 1, false>), grid, dim3(256), 0, st, p);
        else if (V <= 1024 * 8 * 2) hipLaunchKernelGGL((sample_kernel<1024, 2, false>), grid, dim3(1024), 0, st, p);
        else hipLaunchKernelGGL((sample_kernel<1024, 8, false>), grid, dim3(1024), 0, st, p);
    }
    obte_prof_end(prof, st);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}

}  // namespace

extern "C" int obte_sample_logits_bf16(const obte_bf16* logits, int64_t ld, int64_t B, int64_t V, const float* u, float temperature, int32_t top_k, float top_p,
                                       int64_t* token, int32_t* n_kept, obte_stream s) {
    return sample_launch("obte_sample_logits_bf16", logits, ld, B, V, u, temperature, top_k, top_p, nullptr, -1, token, n_kept, s);
}

extern "C" int obte_sample_logits_constrained_bf16(const obte_bf16* logits, int64_t ld, int64_t B, int64_t V, const float* u, float temperature, int32_t top_k,
                                                   float top_p, const uint8_t* allowed, int64_t allowed_ld, int64_t hold_token, const int32_t* emitted,
                                                   int32_t min_emitted, int64_t* token, int32_t* n_kept, obte_stream s) {
    const SpConstraint con{allowed, allowed_ld, emitted, 0, min_emitted};
    return sample_launch("obte_sample_logits_constrained_bf16", logits, ld, B, V, u, temperature, top_k, top_p, &con, hold_token, token, n_kept, s);
}

extern "C" int obte_sample_logits_penalized_bf16(const obte_bf16* logits, int64_t ld, int64_t B, int64_t V, const float* u, float temperature, int32_t top_k,
                                                 float top_p, const uint8_t* allowed, int64_t allowed_ld, int64_t hold_token, const int32_t* emitted,
                                                 int32_t min_emitted, const int64_t* prompt, int64_t prompt_ld, const int32_t* prompt_len, int32_t prompt_max,
                                                 const int64_t* gen, int64_t gen_ld, const int32_t* n_gen, int64_t n_gen_all, int32_t gen_max, float repetition,
                                                 float inv_repetition, float presence, float frequency, int64_t* token, int32_t* n_kept, obte_stream s) {
    const SpConstraint con{allowed, allowed_ld, emitted, 0, min_emitted};
    const SpPenalty pen{prompt, prompt_ld, prompt_len, gen, gen_ld, n_gen, n_gen_all, prompt_max, gen_max, repetition, inv_repetition, presence, frequency};
    return sample_launch("obte_sample_logits_penalized_bf16", logits, ld, B, V, u, temperature, top_k, top_p, &con, hold_token, token, n_kept, s, &pen);
}
