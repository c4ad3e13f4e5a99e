// Speculative decoding, the verification of k drafted tokens per batch row (include/omnibiote_hip_spec.h), in two launches:
//   rows     one workgroup per logits row (the sampler's shape: sample_common.h) leaves the few numbers the decision needs in ws: the
//            row's maximum and lowest argmax, threshold key, integer total, kept count and the drafted token's integer weight.
//   decide   one workgroup per batch row: thread 0 walks the k acceptance tests on those numbers (exact, in 128-bit integers), then the
//            workgroup reads p[a] — and q[a] for the residual — once more, 8 columns per lane and in the sampler's index order, and
//            draws in integer prefix sums as the sampler does: per-wave totals -> the wave that holds the target -> one wave scan per
//            group of chunks -> the lane walks its 8 columns.
// CON: the restricted form (include/omnibiote_hip_constrain.h) — both launches clear the excluded keys of p[b, j] and q[b, j] as they load them.
// PT: the point form (include/omnibiote_hip_lookup.h) — the draft of position j is the token draft[b, j] itself and no q exists.  What the
// other form computes of the row that is 0 at x and -inf elsewhere is known without reading it — total 2^40, x's weight 2^40, every
// other column's 0, and nothing at all for an x outside [0, V) — so `rows` runs over p's k + 1 rows only and `decide` puts those
// integers where it would have loaded them.
#include "sample_common.h"
#include "../../include/omnibiote_hip_lookup.h"

namespace {

constexpr int SV_MAX_K = 31;

struct SpecRow {       // what `rows` leaves per logits row: 32 bytes
    u64 total;         // the kept set's integer mass (0: nothing to sample, or a greedy call)
    u64 wx;            // the drafted token's weight (0: not kept, out of range, or the row has no drafted token)
    uint32_t best;     // maximum key << 16 | (65535 - its lowest column); 0: no entry above -inf that is not NaN
    uint32_t thr;      // threshold key of the kept set
    uint32_t kept;     // size of the kept set
    uint32_t pad;
};

struct SpecParams {
    const bf16* p;
    const bf16* q;
    int64_t ld_p, ld_q;
    const int64_t* draft;
    const float* u_accept;
    const float* u_draw;
    SpecRow* rows;
    int32_t* n_accept;
    int64_t* token;
    float scale;      // log2(e) / temperature
    float top_p;
    int32_t k, V, top_k, greedy;
    SpConstraint con;   // read by the CON kernels only
};

// Logits row r of batch row b's 2 k + 1 (k + 1 when greedy): r <= k is p[b, r], beyond it q[b, r - k - 1]; `j` the position whose drafted
// token the row is asked about (-1: none, p[b, k])
__device__ __forceinline__ const bf16* sv_row(const SpecParams& a, int64_t b, int r, int& j) {
    if (r <= a.k) {
        j = r < a.k ? r : -1;
        return a.p + (b * (a.k + 1) + r) * a.ld_p;
    }
    j = r - a.k - 1;
    return a.q + (b * a.k + j) * a.ld_q;
}

template <int NT, int R, bool CON, bool PT>
__global__ __launch_bounds__(NT) void spec_rows_kernel(SpecParams a) {
    __shared__ u64 hist[SP_BINS];
    __shared__ u64 hist2[16];
    __shared__ u64 red[NT / 64];
    __shared__ u64 red_n[NT / 64];
    __shared__ u64 sel[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = a.greedy || PT ? a.k + 1 : 2 * a.k + 1;
    const int64_t b = blockIdx.x / per;
    const int r = (int)(blockIdx.x % per);
    int j;
    const bf16* x = sv_row(a, b, r, j);
    const int V = a.V;
    const int chunk0 = wave * R * 64 + lane;
    SpecRow* out = a.rows + blockIdx.x;

    uint32_t k[R][4];
    SpRowMask rm{nullptr, -1};
    if (CON) {
        rm = sp_row_mask(a.con, b, r <= a.k ? r : r - a.k - 1);   // the drafted position of the row: p[b, r] or q[b, r - k - 1]
        sp_load_row_masked<R>(x, chunk0, V, rm, k);
    } else {
        sp_load_row<R>(x, chunk0, V, k);
    }
    const uint32_t best = sp_row_max<NT, R>(k, chunk0, red);
    const uint32_t maxkey = best >> 16;
    if (maxkey == 0 || a.greedy) {
        if (tid == 0) { out->total = 0; out->wx = 0; out->best = best; out->thr = 0; out->kept = maxkey ? 1u : 0u; out->pad = 0; }
        return;
    }
    const float maxv = sp_val(maxkey), scale = a.scale;
    const uint32_t thr = sp_threshold<NT, R>(k, maxkey, maxv, scale, V, a.top_k, a.top_p, hist, hist2, red, sel);
    u64 mass, base, total, n;
    sp_row_mass<NT, R>(k, thr, maxkey, maxv, scale, red, red_n, mass, base, total, n);
    if (tid == 0) {
        u64 wx = 0;
        if (j >= 0) {
            const int64_t t = a.draft[b * a.k + j];
            if (t >= 0 && t < V) {   // (any other value is never an index)
                uint32_t key = sp_key(reinterpret_cast<const uint16_t*>(x)[t]);
                if (CON && sp_excluded(rm, (int)t)) key = 0;
                if (key >= thr) wx = sp_weight(key, maxkey, maxv, scale);   // thr >= 1: key 0 is never kept
            }
        }
        out->total = total; out->wx = wx; out->best = best; out->thr = thr; out->kept = (uint32_t)n; out->pad = 0;
    }
}

// ---- 128-bit unsigned integers, as far as the decision needs them ----
struct u128 {
    u64 hi, lo;
};
__device__ __forceinline__ u128 mul64(u64 x, u64 y) { return u128{__umul64hi(x, y), x * y}; }
__device__ __forceinline__ bool lt128(u128 x, u128 y) { return x.hi < y.hi || (x.hi == y.hi && x.lo < y.lo); }
// x << s for 0 <= s < 128; `lost`: bits were shifted out
__device__ __forceinline__ u128 shl128(u128 x, int s, bool& lost) {
    u128 r = x;
    if (s >= 64) { lost = x.hi != 0 || (s > 64 && (x.lo >> (128 - s)) != 0); r.hi = x.lo << (s - 64); r.lo = 0; }
    else if (s > 0) { lost = (x.hi >> (64 - s)) != 0; r.hi = (x.hi << s) | (x.lo >> (64 - s)); r.lo = x.lo << s; }
    else lost = false;
    return r;
}

// u < (wp / tp) / (wq / tq) for wp, wq > 0: with u = m 2^e, m 2^e (wq tp) < wp tq exactly.  wq tp < 2^97, m < 2^24.
__device__ __forceinline__ bool sv_accept(float u, u64 wp, u64 tp, u64 wq, u64 tq) {
    if (!(u > 0.0f)) return true;   // NaN, negative, zero: 0 < the ratio
    const uint32_t bits = __builtin_bit_cast(uint32_t, u);
    const int ex = (int)((bits >> 23) & 0xFFu);
    if (ex == 0xFF) return false;   // +inf
    const u64 m = ex ? ((bits & 0x7FFFFFu) | 0x800000u) : (bits & 0x7FFFFFu);
    const int e = (ex ? ex : 1) - 150;   // u = m 2^e, -149 <= e <= 104
    const u128 num = mul64(wp, tq), den = mul64(wq, tp);
    u128 lhs = mul64(den.lo, m);
    lhs.hi += den.hi * m;            // (den.hi < 2^33: no carry is lost)
    bool lost;
    if (e < 0) {                     // lhs < num 2^-e
        if (-e >= 128) return true;  // num >= 1 and lhs < 2^121
        const u128 rhs = shl128(num, -e, lost);
        return lost || lt128(lhs, rhs);
    }
    const u128 l2 = shl128(lhs, e, lost);   // e <= 104 < 128
    return !lost && lt128(l2, num);
}

__device__ __forceinline__ int sv_bits(u64 t) { return 64 - __clzll((long long)t); }

// r = floor(max(0, wp tq - wq tp) / 2^S), 20 <= S <= 52 (spec header: the residual's one rounding)
__device__ __forceinline__ u64 sv_residual(u64 wp, u64 tq, u64 wq, u64 tp, int S) {
    const u128 x = mul64(wp, tq), y = mul64(wq, tp);
    if (!lt128(y, x)) return 0;
    const u64 lo = x.lo - y.lo, hi = x.hi - y.hi - (x.lo < y.lo ? 1ull : 0ull);
    return (lo >> S) | (hi << (64 - S));   // no bit is lost: wp tq < 2^(40 + bits(tq)), so the quotient is below 2^(102 - bits(tp)) <= 2^61
}

struct SvSide {        // one logits row as the draw reads it
    const bf16* x;
    SpRowMask rm;      // (CON only)
    uint32_t maxkey, thr;
    float maxv;
    int point;         // (PT only, the draft's side) the one column of weight 2^40
};

// the weights of chunk c's 8 columns: the kept entries' fixed-point weights of `P`, or with RES the residual against `Q`
template <bool RES, bool CON, bool PT>
__device__ __forceinline__ void sv_chunk(const SvSide& P, const SvSide& Q, int c, int nch, int V, float scale, u64 tp, u64 tq, int S, u64 (&w)[8]) {
    uint32_t kp[4], kq[4] = {0u, 0u, 0u, 0u};
    if (CON) {   // P and Q are rows of one drafted position: one restriction
        const uint32_t bits = sp_mask_byte(P.rm, c, nch);
        sp_load_chunk_masked(P.x, c, nch, V, bits, kp);
        if (RES) sp_load_chunk_masked(Q.x, c, nch, V, bits, kq);
    } else {
        sp_load_chunk(P.x, c, nch, V, kp);
        if (RES && !PT) sp_load_chunk(Q.x, c, nch, V, kq);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t a = (i & 1) ? kp[i >> 1] >> 16 : kp[i >> 1] & 0xFFFFu;
        const u64 wp = a >= P.thr ? sp_weight(a, P.maxkey, P.maxv, scale) : 0ull;
        if (RES) {
            const uint32_t bq = (i & 1) ? kq[i >> 1] >> 16 : kq[i >> 1] & 0xFFFFu;
            const u64 wq = PT ? (c * 8 + i == Q.point ? SP_ONE : 0ull) : bq >= Q.thr ? sp_weight(bq, Q.maxkey, Q.maxv, scale) : 0ull;
            w[i] = sv_residual(wp, tq, wq, tp, S);
        } else {
            w[i] = wp;
        }
    }
}

// The draw over the row's V entries in index order, weights by sv_chunk<RES>: wave w owns chunks [w R 64, (w + 1) R 64), group g of them
// holds chunk (w R + g) 64 + lane.  Returns the row's total; with `find` (total > 0) the lane that holds the target writes the token.
template <int NT, bool RES, bool CON, bool PT>
__device__ __forceinline__ u64 sv_draw(const SvSide& P, const SvSide& Q, int V, float scale, u64 tp, u64 tq, int S, float u, bool find, int fallback,
                                       int64_t* token, u64* red) {
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = (V + 7) >> 3;
    const int R = (nch + NT - 1) / NT;
    const int chunk0 = wave * R * 64 + lane;
    u64 w[8];
    u64 mass = 0;
    for (int g = 0; g < R; ++g) {
        sv_chunk<RES, CON, PT>(P, Q, chunk0 + g * 64, nch, V, scale, tp, tq, S, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) mass += w[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mass += __shfl_xor(mass, o, 64);
    __syncthreads();
    if (lane == 0) red[wave] = mass;
    __syncthreads();
    u64 base = 0, total = 0;
#pragma unroll 2
    for (int v = 0; v < NW; ++v) {
        const u64 r = red[v];
        base += v < wave ? r : 0;
        total += r;
    }
    if (!find || total == 0) return total;
    const u64 target = sp_draw_target(u, total);
    if (!(base <= target && target < base + mass)) return total;   // (mass: the wave's total after the reduction) one wave goes on
    u64 run = base;
    for (int g = 0; g < R; ++g) {
        const int c = chunk0 + g * 64;
        sv_chunk<RES, CON, PT>(P, Q, c, nch, V, scale, tp, tq, S, w);
        u64 sj = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) sj += w[i];
        const u64 inc = sp_wave_scan(sj);
        const u64 tot = __shfl(inc, 63, 64);
        if (target < run + tot) {
            const u64 hit = __ballot(run + inc > target);
            if (lane == __ffsll((long long)hit) - 1) {
                u64 cum = run + inc - sj;
                int tok = -1;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    cum += w[i];
                    if (tok < 0 && cum > target) tok = c * 8 + i;
                }
                *token = tok < 0 ? fallback : tok;
            }
            break;   // (wave-uniform: run, tot and target are)
        }
        run += tot;
    }
    return total;
}

template <int NT, bool CON, bool PT>
__global__ __launch_bounds__(NT) void spec_decide_kernel(SpecParams a) {
    __shared__ u64 red[NT / 64];
    __shared__ int sh_a;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int k = a.k, per = a.greedy || PT ? k + 1 : 2 * k + 1;
    const SpecRow* rows = a.rows + b * per;
    if (tid == 0) {
        int n = 0;
        for (; n < k; ++n) {
            const SpecRow rp = rows[n];
            if (a.greedy) {
                const int64_t want = (rp.best >> 16) ? 65535 - (int)(rp.best & 0xFFFFu) : 0;
                if (a.draft[b * k + n] != want) break;
                continue;
            }
            if (rp.wx == 0) break;                       // P(x) = 0 never stands
            if (PT) {                                    // (x is inside [0, V): Q(x) = 2^40 / 2^40)
                if (!sv_accept(a.u_accept[b * k + n], rp.wx, rp.total, SP_ONE, SP_ONE)) break;
                continue;
            }
            const SpecRow rq = rows[k + 1 + n];
            if (rq.wx == 0) continue;                    // Q(x) = 0 < P(x) stands
            if (!sv_accept(a.u_accept[b * k + n], rp.wx, rp.total, rq.wx, rq.total)) break;
        }
        sh_a = n;
        a.n_accept[b] = n;
    }
    __syncthreads();
    const int n = sh_a;
    const SpecRow rp = rows[n];
    const uint32_t maxkey = rp.best >> 16;
    const int argmax = 65535 - (int)(rp.best & 0xFFFFu);
    if (maxkey == 0 || a.greedy) {   // nothing to sample: token 0
        if (tid == 0) a.token[b] = maxkey ? argmax : 0;
        return;
    }
    int unused;
    SvSide P, Q;
    P.x = sv_row(a, b, n, unused); P.maxkey = maxkey; P.thr = rp.thr; P.maxv = sp_val(maxkey);
    P.rm = CON ? sp_row_mask(a.con, b, n) : SpRowMask{nullptr, -1};
    P.point = -1;
    Q = P;
    const float u = a.u_draw[b];
    const u64 tp = rp.total;
    if (PT) {
        if (n < k) {
            const int64_t t = a.draft[b * k + n];
            if (t >= 0 && t < a.V) {     // (any other value: the draft row holds nothing, the residual is P)
                Q.point = (int)t;
                const int S = sv_bits(tp) + sv_bits(SP_ONE) - 62;
                if (sv_draw<NT, true, CON, true>(P, Q, a.V, a.scale, tp, SP_ONE, S, u, true, argmax, a.token + b, red) > 0) return;
            }
        }
    } else if (n < k) {
        const SpecRow rq = rows[k + 1 + n];
        if (rq.total > 0) {          // (0: the draft row holds nothing to sample: Q = 0 everywhere, the residual is P)
            Q.x = sv_row(a, b, k + 1 + n, unused); Q.maxkey = rq.best >> 16; Q.thr = rq.thr; Q.maxv = sp_val(Q.maxkey);
            const int S = sv_bits(tp) + sv_bits(rq.total) - 62;
            if (sv_draw<NT, true, CON, false>(P, Q, a.V, a.scale, tp, rq.total, S, u, true, argmax, a.token + b, red) > 0) return;
        }
    }
    sv_draw<NT, false, CON, false>(P, P, a.V, a.scale, tp, 0, 0, u, true, argmax, a.token + b, red);
}

int64_t rows_of(int64_t B, int64_t k, bool greedy) { return B * (greedy ? k + 1 : 2 * k + 1); }

template <bool CON, bool PT>
void spec_launch(const SpecParams& a, int64_t B, int64_t k, int64_t V, bool greedy, hipStream_t st) {
    const dim3 grid((unsigned)rows_of(B, k, greedy || PT)), gridb((unsigned)B);
    if (V <= 256 * 8) {
        hipLaunchKernelGGL((spec_rows_kernel<256, 1, CON, PT>), grid, dim3(256), 0, st, a);
        hipLaunchKernelGGL((spec_decide_kernel<256, CON, PT>), gridb, dim3(256), 0, st, a);
    } else {
        if (V <= 1024 * 8 * 2) hipLaunchKernelGGL((spec_rows_kernel<1024, 2, CON, PT>), grid, dim3(1024), 0, st, a);
        else hipLaunchKernelGGL((spec_rows_kernel<1024, 8, CON, PT>), grid, dim3(1024), 0, st, a);
        hipLaunchKernelGGL((spec_decide_kernel<1024, CON, PT>), gridb, dim3(1024), 0, st, a);
    }
}

int64_t ws_bytes_of(int64_t B, int64_t k, bool point = false) {
    if (B < 1 || k < 1 || k > SV_MAX_K || B >= (1ll << 24)) return 0;
    return rows_of(B, k, point) * (int64_t)sizeof(SpecRow);
}

// the three entry points: `con` NULL and `point` false is obte_spec_verify_bf16 itself; `point`: no q, the draft is draft[b, j] itself
int spec_verify(const char* who, bool point, const obte_bf16* p, int64_t ld_p, const obte_bf16* q, int64_t ld_q, const int64_t* draft, int64_t B, int64_t k, int64_t V,
                const float* u_accept, const float* u_draw, float temperature, int32_t top_k, float top_p, const SpConstraint* con, int64_t hold_token,
                int32_t* n_accept, int64_t* token, void* ws, int64_t ws_bytes, obte_stream s) {
    static_assert(sizeof(SpecRow) == 32, "the workspace holds 32 bytes per logits row");
    OBTE_REQUIRE(p && draft && n_accept && token && ws, "%s: null pointer (p, draft, n_accept, token, ws)", who);
    OBTE_REQUIRE(B >= 1 && B < (1ll << 24) && k >= 1 && V >= 1, "%s: B, k and V must be at least 1 (B=%lld k=%lld V=%lld)", who, (long long)B, (long long)k,
                 (long long)V);
    if (V > SP_MAX_V) {
        obte_set_error("%s: V = %lld exceeds the %d columns a workgroup holds in registers", who, (long long)V, SP_MAX_V);
        return OBTE_EUNSUPPORTED;
    }
    if (k > SV_MAX_K) {
        obte_set_error("%s: k = %lld exceeds %d drafted tokens (k + 1 queries fill the extend kernel's tile of 32)", who, (long long)k, SV_MAX_K);
        return OBTE_EUNSUPPORTED;
    }
    OBTE_REQUIRE(temperature >= 0.f && isfinite(temperature), "%s: temperature must be finite and not negative", who);
    OBTE_REQUIRE(top_p > 0.f && top_p <= 1.f, "%s: top_p must lie in (0, 1]", who);
    const bool greedy = !u_accept || !u_draw || temperature == 0.f || top_k == 1;
    OBTE_REQUIRE(q || greedy || point, "%s: null pointer (q): only a greedy call goes without the draft's logits", who);
    OBTE_REQUIRE(ld_p % 8 == 0, "%s: ld_p must be a multiple of 8 (16-byte rows), got %lld", who, (long long)ld_p);
    OBTE_REQUIRE(ld_p >= V, "%s: ld_p %lld is smaller than V %lld", who, (long long)ld_p, (long long)V);
    OBTE_REQUIRE_ALIGNED(who, p, "p", 16);
    if (q) {
        OBTE_REQUIRE(ld_q % 8 == 0, "%s: ld_q must be a multiple of 8 (16-byte rows), got %lld", who, (long long)ld_q);
        OBTE_REQUIRE(ld_q >= V, "%s: ld_q %lld is smaller than V %lld", who, (long long)ld_q, (long long)V);
        OBTE_REQUIRE_ALIGNED(who, q, "q", 16);
    }
    OBTE_REQUIRE_ALIGNED(who, draft, "draft", 8);
    OBTE_REQUIRE_ALIGNED(who, u_accept, "u_accept", 4);
    OBTE_REQUIRE_ALIGNED(who, u_draw, "u_draw", 4);
    OBTE_REQUIRE_ALIGNED(who, n_accept, "n_accept", 4);
    OBTE_REQUIRE_ALIGNED(who, token, "token", 8);
    OBTE_REQUIRE_ALIGNED(who, ws, "ws", 8);
    const int64_t need = ws_bytes_of(B, k, point);
    OBTE_REQUIRE(ws_bytes >= need, "%s: workspace of %lld bytes, %lld needed (%s)", who, (long long)ws_bytes, (long long)need,
                 point ? "obte_spec_verify_point_ws_bytes" : "obte_spec_verify_ws_bytes");
    SpecParams a;
    a.p = (const bf16*)p; a.q = (const bf16*)q; a.ld_p = ld_p; a.ld_q = ld_q; a.draft = draft; a.u_accept = u_accept; a.u_draw = u_draw;
    a.rows = (SpecRow*)ws; a.n_accept = n_accept; a.token = token;
    a.k = (int32_t)k; a.V = (int32_t)V; a.top_k = top_k; a.top_p = top_p;
    a.greedy = greedy ? 1 : 0;
    a.scale = greedy ? 1.f : (float)(1.4426950408889634 / (double)temperature);
    a.con = SpConstraint{nullptr, 0, nullptr, -1, 0};
    if (con) {
        const int rc = sp_check_constraint(who, *con, hold_token, V, &a.con);
        if (rc != OBTE_OK) return rc;
    }
    hipStream_t st = (hipStream_t)s;
    const int prof = obte_prof_begin(st, point ? 123 : 115, B, k, V);
    if (point) spec_launch<false, true>(a, B, k, V, greedy, st);
    else if (con) spec_launch<true, false>(a, B, k, V, greedy, st);
    else spec_launch<false, false>(a, B, k, V, greedy, st);
    obte_prof_end(prof, st);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}

}  // namespace

extern "C" int64_t obte_spec_verify_ws_bytes(int64_t B, int64_t k) { return ws_bytes_of(B, k); }

extern "C" int obte_spec_verify_bf16(const obte_bf16* p, int64_t ld_p, const obte_bf16* q, int64_t ld_q, const int64_t* draft, int64_t B, int64_t k, int64_t V,
                                     const float* u_accept, const float* u_draw, float temperature, int32_t top_k, float top_p, int32_t* n_accept,
                                     int64_t* token, void* ws, int64_t ws_bytes, obte_stream s) {
    return spec_verify("obte_spec_verify_bf16", false, p, ld_p, q, ld_q, draft, B, k, V, u_accept, u_draw, temperature, top_k, top_p, nullptr, -1, n_accept, token, ws,
                       ws_bytes, s);
}

extern "C" int obte_spec_verify_constrained_bf16(const obte_bf16* p, int64_t ld_p, const obte_bf16* q, int64_t ld_q, const int64_t* draft, int64_t B, int64_t k,
                                                 int64_t V, const float* u_accept, const float* u_draw, float temperature, int32_t top_k, float top_p,
                                                 const uint8_t* allowed, int64_t allowed_ld, int64_t hold_token, const int32_t* emitted, int32_t min_emitted,
                                                 int32_t* n_accept, int64_t* token, void* ws, int64_t ws_bytes, obte_stream s) {
    const SpConstraint con{allowed, allowed_ld, emitted, 0, min_emitted};
    return spec_verify("obte_spec_verify_constrained_bf16", false, p, ld_p, q, ld_q, draft, B, k, V, u_accept, u_draw, temperature, top_k, top_p, &con, hold_token,
                       n_accept, token, ws, ws_bytes, s);
}

extern "C" int64_t obte_spec_verify_point_ws_bytes(int64_t B, int64_t k) { return ws_bytes_of(B, k, true); }

extern "C" int obte_spec_verify_point_bf16(const obte_bf16* p, int64_t ld_p, const int64_t* draft, int64_t B, int64_t k, int64_t V, const float* u_accept,
                                           const float* u_draw, float temperature, int32_t top_k, float top_p, int32_t* n_accept, int64_t* token, void* ws,
                                           int64_t ws_bytes, obte_stream s) {
    return spec_verify("obte_spec_verify_point_bf16", true, p, ld_p, nullptr, 0, draft, B, k, V, u_accept, u_draw, temperature, top_k, top_p, nullptr, -1, n_accept,
                       token, ws, ws_bytes, s);
}
