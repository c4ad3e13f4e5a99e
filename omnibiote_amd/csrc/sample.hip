// Next-token sampling on the device (include/omnibiote_hip_sample.h): temperature, top-k, top-p, softmax and the draw, one workgroup
// per row of bf16 logits, the row read once and held in registers as order-preserving 16-bit keys for every pass (sample_common.h:
// the load, the maximum, the select and the weights).
//   draw     per-wave integer totals -> the wave that holds floor(u total); there one wave scan per register group finds the lane,
//            and the lane walks its 8 columns.
// CON: the restricted form (include/omnibiote_hip_constrain.h) — the load clears the excluded keys, everything after it is the same code.
#include "sample_common.h"

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

template <int NT, int R, bool CON>
__global__ __launch_bounds__(NT) void sample_kernel(SampleParams p) {
    __shared__ u64 hist[SP_BINS];
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
    if (CON) sp_load_row_masked<R>(x, chunk0, V, sp_row_mask(p.con, row, 0), k);
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

// both entry points: `con` NULL is obte_sample_logits_bf16 itself
int sample_launch(const char* who, const obte_bf16* logits, int64_t ld, int64_t B, int64_t V, const float* u, float temperature, int32_t top_k, float top_p,
                  const SpConstraint* con, int64_t hold_token, int64_t* token, int32_t* n_kept, obte_stream s) {
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
    SampleParams p;
    p.logits = (const bf16*)logits; p.ld = ld; p.u = u; p.token = token; p.n_kept = n_kept;
    p.V = (int32_t)V; p.top_k = top_k; p.top_p = top_p;
    p.greedy = (!u || temperature == 0.f || top_k == 1) ? 1 : 0;
    p.scale = p.greedy ? 1.f : (float)(1.4426950408889634 / (double)temperature);
    p.con = SpConstraint{nullptr, 0, nullptr, -1, 0};
    if (con) {
        const int rc = sp_check_constraint(who, *con, hold_token, V, &p.con);
        if (rc != OBTE_OK) return rc;
    }
    hipStream_t st = (hipStream_t)s;
    const int prof = obte_prof_begin(st, 114, B, V, p.greedy);
    const dim3 grid((unsigned)B);
    if (con) {
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
