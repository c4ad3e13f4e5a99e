// Many samples per prompt (include/omnibiote_hip_shared.h): one query per (row, head) over a key/value cache whose first n_prefix
// positions are shared by the G rows of a group.  B = P G rows, row b = p G + g; the prefix is a layer cache of P rows, the suffix a
// layer cache of B rows whose slot i is the row's own position n_prefix + i (both in attention_decode.hip's layout).
//
// obte_attn_decode_shared is three launches, none of them a new tile loop:
//   - the prefix: attn_extend_kernel<.., GROUP> (attention_extend.hip) with the group read as the chunk.  The G queries of (p, h) go
//     through the MFMA 32 at a time against keys that are loaded once per tile instead of once per row — the replicated cache reads
//     4 hs B H n bytes a step, this 4 hs P H ceil(G / 32) n_prefix.  Always partials: (m, l, O^T) per (p, h, tile, split).
//   - the suffix: attn_decode_kernel<.., PARTIAL> (attention_decode.hip) on the rows' own positions, partials at one split too.
//   - the combine below: one workgroup per (b, h), thread d owning dimension d; the maximum over the row's prefix partials and then its
//     suffix partials, made finite, then the sums in that order, each partial rescaled to it; one rounding of o.  n_prefix >= 1 puts a
//     key in the first prefix split, so l > 0; the guard for l = 0 stays, as in every combine of this library.
// A row's result is a function of its own column of a prefix tile (an MFMA column is computed from that column's query alone), its own
// suffix partials and the two split counts: the same bits at every G and every P.  No atomics, no flags.
#include "common.h"

namespace {

constexpr int QT = 32;            // queries per prefix tile (attention_extend.hip's EXT_QT)
constexpr int64_t TARGET_WGS = 256;   // 1 per CU, as the decode and extend rules
constexpr int64_t MIN_KEYS = 256;     // a prefix split is worth its workgroup with two 32-key tiles per wave: the second's loads fly under the first's softmax

// grid B * H, HS threads.  pre: [P H][tiles][ps][HS / 2 + 2][64]; suf: [B H][ss][HS + DEC_PAD] (ss = 0: no suffix)
template <int HS>
__global__ __launch_bounds__(HS) void attn_shared_combine_kernel(const float* __restrict__ pre, const float* __restrict__ suf, bf16* __restrict__ o,
                                                                 float* __restrict__ lse, int H, int G, int tiles, int ps, int ss) {
    constexpr int NR = HS / 2, PART = (NR + 2) * 64, SPART = HS + DEC_PAD;
    const int bh = blockIdx.x, d = threadIdx.x;
    const int b = bh / H, h = bh % H, p = b / G, j = b % G;
    const int dd = d & 31;
    const int reg = 16 * (d >> 5) + (dd & 3) + 4 * (dd >> 3);   // the inverse of acc_row (attn_common.h): row dd of a 32 x 32 accumulator tile
    const int lane = (j % QT) + 32 * ((dd >> 2) & 1);
    const float* pp = pre + (((int64_t)p * H + h) * tiles + j / QT) * ps * PART + lane;
    const float* sp = suf + (int64_t)bh * ss * SPART;
    float m = -INFINITY;
    for (int s = 0; s < ps; ++s) m = fmaxf(m, pp[(int64_t)s * PART + NR * 64]);
    for (int s = 0; s < ss; ++s) m = fmaxf(m, sp[s * SPART + HS]);
    const float ms = m == -INFINITY ? 0.f : m;
    float l = 0.f, acc = 0.f;
    for (int s = 0; s < ps; ++s) {
        const float* w = pp + (int64_t)s * PART;
        const float wt = __builtin_amdgcn_exp2f(w[NR * 64] - ms);
        l += w[(NR + 1) * 64] * wt;
        acc += w[reg * 64] * wt;
    }
    for (int s = 0; s < ss; ++s) {
        const float* w = sp + s * SPART;
        const float wt = __builtin_amdgcn_exp2f(w[HS] - ms);
        l += w[HS + 1] * wt;
        acc += w[d] * wt;
    }
    o[(int64_t)bh * HS + d] = f2bf(l == 0.f ? 0.f : acc / l);
    if (lse && d == 0) lse[bh] = l == 0.f ? -INFINITY : (m + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;   // v_log_f32 is log2
}

bool shape_ok(int64_t P, int64_t G, int32_t n_head, int32_t head_dim) {
    return P > 0 && G > 0 && G < (1ll << 20) && P <= 65535 && n_head > 0 && n_head <= 1024 && (head_dim == 64 || head_dim == 128) && P * n_head <= 65535 &&
           P * G * n_head <= 65535;
}
int64_t tiles_of(int64_t G) { return cdiv64(G, QT); }
int64_t prefix_bound(int64_t P, int64_t G, int32_t n_head) {
    int64_t n = cdiv64(TARGET_WGS, P * n_head * tiles_of(G));
    if (n > OBTE_ATTN_SHARED_MAX_SPLITS) n = OBTE_ATTN_SHARED_MAX_SPLITS;
    return n < 1 ? 1 : n;
}
int64_t pre_bytes(int64_t P, int64_t G, int32_t n_head, int32_t head_dim, int64_t ps) { return P * n_head * tiles_of(G) * ps * obte_ext_part_floats(head_dim) * 4; }
int64_t suf_bytes(int64_t B, int32_t n_head, int32_t head_dim, int64_t ss) { return B * n_head * ss * (int64_t)(head_dim + DEC_PAD) * 4; }

}  // namespace

// The default prefix split count: decode's rule (a split is worth its workgroup and its share of the combine only with MIN_KEYS keys of
// its own, more than one workgroup per CU buys nothing) on the workgroups of every (p, h, tile).
extern "C" int obte_attn_shared_prefix_splits(int64_t P, int64_t G, int32_t n_head, int32_t head_dim, int64_t n_prefix) {
    if (!shape_ok(P, G, n_head, head_dim) || n_prefix < 1) return 1;
    const int64_t by_keys = n_prefix / MIN_KEYS, bound = prefix_bound(P, G, n_head);
    const int64_t n = by_keys < bound ? by_keys : bound;
    return n < 1 ? 1 : (int)n;
}

extern "C" int64_t obte_attn_decode_shared_ws_bytes(int64_t P, int64_t G, int32_t n_head, int32_t head_dim, int32_t prefix_splits, int32_t suffix_splits) {
    if (!shape_ok(P, G, n_head, head_dim) || prefix_splits < 0 || prefix_splits > OBTE_ATTN_SHARED_MAX_SPLITS || suffix_splits < 0 ||
        suffix_splits > OBTE_ATTN_DECODE_MAX_SPLITS)
        return 0;
    const int64_t ps = prefix_splits > 0 ? prefix_splits : prefix_bound(P, G, n_head);
    const int64_t ss = suffix_splits > 0 ? suffix_splits : obte_attn_decode_splits(P * G, n_head, head_dim, (1ll << 24) - 1);   // (the rule's bound by fill alone)
    return pre_bytes(P, G, n_head, head_dim, ps) + suf_bytes(P * G, n_head, head_dim, ss);
}

namespace {

// obte_attn_decode_shared (ancestry null) and obte_attn_decode_beam (include/omnibiote_hip_beam.h: the suffix launch reads slot j of row b
// from the group's row ancestry[b][j]); who: the entry point named in an error
int decode_shared_on(const char* who, bool beam, const obte_bf16* q, int64_t q_ld, const obte_bf16* prefix_cache, int64_t P, int64_t T_pre, int64_t n_prefix,
                     const obte_bf16* suffix_cache, int64_t G, int64_t T_suf, int64_t n_suffix, const int32_t* ancestry, obte_bf16* o, float* lse, int32_t n_head,
                     int32_t head_dim, float scale, int32_t prefix_splits, int32_t suffix_splits, void* ws, int64_t ws_bytes, obte_stream s) {
    OBTE_REQUIRE(q && prefix_cache && o && (suffix_cache || n_suffix == 0) && (!beam || ancestry || n_suffix == 0), "%s: null pointer", who);
    OBTE_REQUIRE(shape_ok(P, G, n_head, head_dim) && T_pre > 0 && T_pre < (1ll << 24) && T_suf >= 0 && T_suf < (1ll << 24),
                 "%s: bad shape (head_dim 64 or 128, P * n_head and P * G * n_head <= 65535)", who);
    OBTE_REQUIRE(n_prefix >= 1 && n_prefix <= T_pre, "%s: n_prefix = %lld outside [1, T_pre = %lld]", who, (long long)n_prefix, (long long)T_pre);
    OBTE_REQUIRE(n_suffix >= 0 && n_suffix <= T_suf, "%s: n_suffix = %lld outside [0, T_suf = %lld]", who, (long long)n_suffix, (long long)T_suf);
    OBTE_REQUIRE(q_ld >= (int64_t)n_head * head_dim && q_ld % 8 == 0, "%s: q_ld must be a multiple of 8 and at least n_head * head_dim", who);
    OBTE_REQUIRE((((uintptr_t)q | (uintptr_t)prefix_cache | (uintptr_t)suffix_cache | (uintptr_t)o) & 15) == 0 && (((uintptr_t)lse | (uintptr_t)ancestry) & 3) == 0,
                 "%s: q, both caches and o must be 16-byte aligned, lse%s 4-byte aligned", who, beam ? " and ancestry" : "");
    OBTE_REQUIRE(prefix_splits >= 0 && prefix_splits <= OBTE_ATTN_SHARED_MAX_SPLITS, "%s: prefix_splits = %d outside [0, %d]", who, prefix_splits,
                 OBTE_ATTN_SHARED_MAX_SPLITS);
    OBTE_REQUIRE(suffix_splits >= 0 && suffix_splits <= OBTE_ATTN_DECODE_MAX_SPLITS, "%s: suffix_splits = %d outside [0, %d]", who, suffix_splits,
                 OBTE_ATTN_DECODE_MAX_SPLITS);
    const int64_t B = P * G;
    const int ps = prefix_splits > 0 ? prefix_splits : obte_attn_shared_prefix_splits(P, G, n_head, head_dim, n_prefix);
    const int ss = n_suffix == 0 ? 0 : suffix_splits > 0 ? suffix_splits : obte_attn_decode_splits(B, n_head, head_dim, n_suffix);
    const int64_t pre = pre_bytes(P, G, n_head, head_dim, ps), need = pre + suf_bytes(B, n_head, head_dim, ss);
    OBTE_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0,
                 "%s: %d prefix and %d suffix splits need a 16-byte aligned workspace of %lld bytes, got %lld", who, ps, ss, (long long)need,
                 (long long)(ws ? ws_bytes : 0));
    const hipStream_t st = (hipStream_t)s;
    const float qscale = scale * 1.4426950408889634f;
    const int tiles = (int)tiles_of(G), BH = (int)(B * n_head);
    float* pre_part = (float*)ws;
    float* suf_part = (float*)((char*)ws + pre);
    int prof = obte_prof_begin(st, 106, P * n_head * tiles, n_prefix, head_dim);   // cache bytes read = 4 * P * n_head * tiles * n_prefix * head_dim
    obte_attn_extend_group_partials(head_dim, P, (int)G, n_head, ps, (const bf16*)q, q_ld, (const bf16*)prefix_cache, T_pre, (int)n_prefix, qscale, pre_part, st);
    obte_prof_end(prof, st);
    if (ss > 0) {
        prof = obte_prof_begin(st, beam ? 118 : 102, BH, n_suffix, head_dim);      // cache bytes read = 4 * BH * n_suffix * head_dim
        obte_attn_decode_partials(head_dim, BH, n_head, ss, (const bf16*)q, q_ld, (const bf16*)suffix_cache, T_suf, (int)n_suffix, qscale, suf_part, st,
                                  beam ? ancestry : nullptr, (int)G);
        obte_prof_end(prof, st);
    }
    prof = obte_prof_begin(st, 107, BH, ps + ss, head_dim);
    if (head_dim == 128)
        hipLaunchKernelGGL(attn_shared_combine_kernel<128>, dim3(BH), dim3(128), 0, st, (const float*)pre_part, (const float*)suf_part, (bf16*)o, lse, n_head, (int)G,
                           tiles, ps, ss);
    else
        hipLaunchKernelGGL(attn_shared_combine_kernel<64>, dim3(BH), dim3(64), 0, st, (const float*)pre_part, (const float*)suf_part, (bf16*)o, lse, n_head, (int)G,
                           tiles, ps, ss);
    obte_prof_end(prof, st);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}

}  // namespace

extern "C" int obte_attn_decode_shared(const obte_bf16* q, int64_t q_ld, const obte_bf16* prefix_cache, int64_t P, int64_t T_pre, int64_t n_prefix,
                                       const obte_bf16* suffix_cache, int64_t G, int64_t T_suf, int64_t n_suffix, obte_bf16* o, float* lse, int32_t n_head,
                                       int32_t head_dim, float scale, int32_t prefix_splits, int32_t suffix_splits, void* ws, int64_t ws_bytes, obte_stream s) {
    return decode_shared_on("obte_attn_decode_shared", false, q, q_ld, prefix_cache, P, T_pre, n_prefix, suffix_cache, G, T_suf, n_suffix, nullptr, o, lse, n_head,
                            head_dim, scale, prefix_splits, suffix_splits, ws, ws_bytes, s);
}

extern "C" int obte_attn_decode_beam(const obte_bf16* q, int64_t q_ld, const obte_bf16* prefix_cache, int64_t P, int64_t T_pre, int64_t n_prefix,
                                     const obte_bf16* suffix_cache, int64_t G, int64_t T_suf, int64_t n_suffix, const int32_t* ancestry, obte_bf16* o, float* lse,
                                     int32_t n_head, int32_t head_dim, float scale, int32_t prefix_splits, int32_t suffix_splits, void* ws, int64_t ws_bytes,
                                     obte_stream s) {
    return decode_shared_on("obte_attn_decode_beam", true, q, q_ld, prefix_cache, P, T_pre, n_prefix, suffix_cache, G, T_suf, n_suffix, ancestry, o, lse, n_head,
                            head_dim, scale, prefix_splits, suffix_splits, ws, ws_bytes, s);
}
