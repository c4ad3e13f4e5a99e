// Beam search, the selection (include/omnibiote_hip_beam.h): per prompt the W best of W V candidates (beam score + log-softmax of a bf16
// row), in two launches and one read of the logits.
//   rows    one workgroup per row, the row held in registers as the sampler holds it (sample_common.h: the masked load, the maximum, the
//           2^40 fixed-point weights, the two-level select).  Its normaliser is the integer sum of the weights at temperature 1; its W
//           best columns by (value descending, column ascending) are the entries above the W-th largest value — compacted in thread
//           order by one block scan — and of the entries AT that value the lowest columns, one block maximum each (the select keeps a
//           tie at the threshold whole; a beam step may take only part of it).  They leave as W packed words (key << 16 | 65535 -
//           column; 0: none) with the row's ln Z, score and state.
//   merge   one workgroup per group, thread t = candidate (beam t / W, place t % W): S in double, one rounding to fp32, a 64-bit sort
//           word (S as an ordered integer, then the lower beam, then the lower token), the rank by counting the larger words in LDS.
//           Ranks < W write the group's rows; the group's threads then copy the parents' ancestry rows.
// No atomics on global memory; the LDS atomics of the select add integers, so nothing depends on the order they arrive in.
#include "sample_common.h"
#include "../../include/omnibiote_hip_beam.h"

namespace {

constexpr uint32_t ROW_LIVE = 0, ROW_DONE = 1, ROW_DEAD = 2;

struct RowStat {       // 16 bytes per row, behind the candidates
    double lnz;
    float score;
    uint32_t maxkey_state;   // maximum's key << 8 | state
};

struct BeamRowParams {
    const bf16* logits;
    int64_t ld;
    const float* score_in;
    const uint8_t* done_in;
    const uint8_t* allowed;
    int64_t allowed_ld;
    uint32_t* cand;    // [B][W]
    RowStat* stat;     // [B]
    int32_t V, W;
};

template <int NT, int R>
__global__ __launch_bounds__(NT) void beam_rows_kernel(BeamRowParams p) {
    __shared__ u64 hist[SP_BINS];
    __shared__ u64 hist2[16];
    __shared__ u64 red[NT / 64];
    __shared__ u64 red_n[NT / 64];
    __shared__ u64 sel[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x;
    const int V = p.V, W = p.W;
    uint32_t* cand = p.cand + row * W;
    const float score = p.score_in[row];
    const bool finite = __builtin_fabsf(score) < INFINITY;   // (false for NaN)
    const uint32_t state = !finite ? ROW_DEAD : p.done_in[row] ? ROW_DONE : ROW_LIVE;
    if (state != ROW_LIVE) {   // (workgroup-uniform) nothing of the row is read
        if (tid < W) cand[tid] = 0u;
        if (tid == 0) p.stat[row] = RowStat{0.0, score, state};
        return;
    }
    const int chunk0 = wave * R * 64 + lane;
    uint32_t k[R][4];
    SpRowMask m;
    m.bits = p.allowed ? p.allowed + row * p.allowed_ld : nullptr;
    m.hold = -1;
    sp_load_row_masked<R>(p.logits + row * p.ld, chunk0, V, m, k);
    const uint32_t best = sp_row_max<NT, R>(k, chunk0, red);
    const uint32_t maxkey = best >> 16;
    if (maxkey == 0) {   // no candidate column
        if (tid < W) cand[tid] = 0u;
        if (tid == 0) p.stat[row] = RowStat{0.0, score, ROW_DEAD};
        return;
    }
    const float maxv = sp_val(maxkey), scale = 1.4426950408889634f;
    u64 mass, base, total, n;
    sp_row_mass<NT, R>(k, 1u, maxkey, maxv, scale, red, red_n, mass, base, total, n);
    if (tid == 0) p.stat[row] = RowStat{log((double)total) - 40.0 * 0.6931471805599453, score, (maxkey << 8) | ROW_LIVE};

    // the W-th largest value (fewer than W entries: 1, below every key that stands for a value)
    const uint32_t thr = sp_select<NT, R, false>(k, 1u, maxkey, maxv, scale, (u64)W, 0.f, hist, hist2, red, sel);
    u64 above = 0;
    sp_each<R>(k, [&](uint32_t key, int) { above += key > thr ? 1u : 0u; });
    u64 n_above;
    u64 pos = sp_block_scan<NT>(above, red, n_above);
    sp_each<R>(k, [&](uint32_t key, int slot) {
        if (key > thr) {
            const int col = (chunk0 + (slot >> 3) * 64) * 8 + (slot & 7);
            if (pos < (u64)W) cand[pos] = (key << 16) | (uint32_t)(65535 - col);
            pos += 1;
        }
    });
    // the entries at the threshold, lowest column first: code = 65536 - column, each round's maximum below the round before's
    uint32_t last = 0x10001u;
    for (int at = (int)n_above; at < W; ++at) {   // (n_above < W whenever thr is a value of the row)
        uint32_t mine = 0;
        sp_each<R>(k, [&](uint32_t key, int slot) {
            const uint32_t code = 65536u - (uint32_t)((chunk0 + (slot >> 3) * 64) * 8 + (slot & 7));
            if (key == thr && code < last) mine = max(mine, code);
        });
        const uint32_t got = sp_block_max<NT>(mine, red);
        if (tid == 0) cand[at] = got ? (thr << 16) | (got - 1u) : 0u;   // (65535 - column = code - 1)
        last = got ? got : 0u;   // nothing left: every later round finds nothing and writes 0
    }
}

struct BeamMergeParams {
    const uint32_t* cand;
    const RowStat* stat;
    const int32_t* anc_in;
    int32_t* anc_out;
    int32_t* parent;
    int64_t* token;
    float* score_out;
    uint8_t* done_out;
    int64_t* token_row;   // token_hist + slot * B
    int64_t T_suf;
    int32_t W, slot, eos;
};

// a float as an integer of the same order, never 0 (-inf: 0x007FFFFF)
__device__ __forceinline__ uint32_t ordered(float f) {
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// NT >= W * W threads, a multiple of 64
template <int NT>
__global__ __launch_bounds__(NT) void beam_merge_kernel(BeamMergeParams p) {
    __shared__ u64 word[NT];
    __shared__ int par[OBTE_BEAM_MAX_WIDTH];
    const int tid = threadIdx.x, W = p.W;
    const int64_t row0 = (int64_t)blockIdx.x * W;
    const int g = tid / W, i = tid % W;
    u64 mine = 0;
    float S = 0.f;
    int tok = 0;
    uint32_t state = ROW_DEAD;
    if (tid < W * W) {
        const RowStat st = p.stat[row0 + g];
        state = st.maxkey_state & 0xFFu;
        if (state == ROW_DONE) {
            if (i == 0) {
                S = st.score;
                tok = p.eos < 0 ? 0 : p.eos;
                mine = 1;
            }
        } else if (state == ROW_LIVE) {
            const uint32_t c = p.cand[(row0 + g) * W + i];
            const uint32_t key = c >> 16, maxkey = st.maxkey_state >> 8;
            if (key) {
                const double dx = key == maxkey ? 0.0 : (double)sp_val(key) - (double)sp_val(maxkey);
                S = (float)((double)st.score + dx - st.lnz);
                tok = 65535 - (int)(c & 0xFFFFu);
                mine = S == -INFINITY ? 0 : 1;   // (x - max below every fp32: no candidate)
            }
        }
        if (mine) mine = ((u64)ordered(S) << 32) | ((u64)(255 - g) << 16) | (u64)(65535 - tok);
    }
    word[tid] = mine;
    if (tid < W) par[tid] = tid;   // a dead rank's parent: the row itself
    __syncthreads();
    int rank = 0, valid = 0;
    for (int j = 0; j < W * W; ++j) {
        const u64 o = word[j];
        rank += o > mine ? 1 : 0;
        valid += o != 0 ? 1 : 0;
    }
    if (mine && rank < W) {
        const int64_t b = row0 + rank;
        p.parent[b] = (int32_t)(row0 + g);
        p.token[b] = tok;
        p.token_row[b] = tok;
        p.score_out[b] = S;
        p.done_out[b] = (state == ROW_DONE || tok == p.eos) ? 1 : 0;
        par[rank] = g;
    }
    if (tid >= valid && tid < W) {
        const int64_t b = row0 + tid;
        const int64_t t = p.eos < 0 ? 0 : p.eos;
        p.parent[b] = (int32_t)b;
        p.token[b] = t;
        p.token_row[b] = t;
        p.score_out[b] = -INFINITY;
        p.done_out[b] = 1;
    }
    __syncthreads();
    const int slot = p.slot;
    for (int e = tid; e < W * slot; e += NT) {
        const int r = e / slot, j = e - r * slot;
        p.anc_out[(row0 + r) * p.T_suf + j] = p.anc_in[(row0 + par[r]) * p.T_suf + j];
    }
    if (tid < W) p.anc_out[(row0 + tid) * p.T_suf + slot] = tid;
}

int64_t cand_bytes(int64_t B, int64_t W) { return (B * W * 4 + 15) / 16 * 16; }
bool shape_ok(int64_t P, int64_t W) { return P >= 1 && W >= 1 && W <= OBTE_BEAM_MAX_WIDTH && P < (1ll << 31) / OBTE_BEAM_MAX_WIDTH; }
bool overlap(const void* a, const void* b, int64_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}

}  // namespace

extern "C" int64_t obte_beam_select_ws_bytes(int64_t P, int64_t W) {
    return shape_ok(P, W) ? cand_bytes(P * W, W) + P * W * (int64_t)sizeof(RowStat) : 0;
}

extern "C" int obte_beam_select_bf16(const obte_bf16* logits, int64_t ld, int64_t P, int64_t W, int64_t V, const float* score_in, const uint8_t* done_in,
                                     int64_t eos_token, const uint8_t* allowed, int64_t allowed_ld, const int32_t* ancestry_in, int64_t T_suf, int64_t slot,
                                     int32_t* parent, int64_t* token, float* score_out, uint8_t* done_out, int32_t* ancestry_out, int64_t* token_hist, void* ws,
                                     int64_t ws_bytes, obte_stream s) {
    const char* who = "obte_beam_select_bf16";
    OBTE_REQUIRE(logits && score_in && done_in && ancestry_in && parent && token && score_out && done_out && ancestry_out && token_hist,
                 "%s: null pointer (logits, score_in, done_in, ancestry_in, parent, token, score_out, done_out, ancestry_out, token_hist)", who);
    OBTE_REQUIRE(P >= 1 && P < (1ll << 31) / OBTE_BEAM_MAX_WIDTH && V >= 1, "%s: P and V must be at least 1 (P=%lld V=%lld)", who, (long long)P, (long long)V);
    OBTE_REQUIRE(W >= 1 && W <= OBTE_BEAM_MAX_WIDTH, "%s: W = %lld outside [1, %d]", who, (long long)W, OBTE_BEAM_MAX_WIDTH);
    if (V > SP_MAX_V) {
        obte_set_error("%s: V = %lld exceeds the %d columns a workgroup holds in registers", who, (long long)V, SP_MAX_V);
        return OBTE_EUNSUPPORTED;
    }
    OBTE_REQUIRE(ld % 8 == 0, "%s: ld must be a multiple of 8 (16-byte rows), got %lld", who, (long long)ld);
    OBTE_REQUIRE(ld >= V, "%s: ld %lld is smaller than V %lld", who, (long long)ld, (long long)V);
    OBTE_REQUIRE_ALIGNED(who, logits, "logits", 16);
    OBTE_REQUIRE(eos_token >= -1 && eos_token < V, "%s: eos_token = %lld outside [-1, V = %lld)", who, (long long)eos_token, (long long)V);
    OBTE_REQUIRE(allowed_ld >= 0, "%s: allowed_ld must not be negative, got %lld", who, (long long)allowed_ld);
    OBTE_REQUIRE(allowed_ld == 0 || allowed_ld >= (V + 7) / 8, "%s: allowed_ld %lld is smaller than the ceil(V / 8) = %lld bytes of a mask row", who,
                 (long long)allowed_ld, (long long)((V + 7) / 8));
    OBTE_REQUIRE(T_suf >= 1 && T_suf < (1ll << 24), "%s: T_suf = %lld outside [1, 2^24)", who, (long long)T_suf);
    OBTE_REQUIRE(slot >= 0 && slot < T_suf, "%s: slot = %lld outside [0, T_suf = %lld)", who, (long long)slot, (long long)T_suf);
    OBTE_REQUIRE_ALIGNED(who, score_in, "score_in", 4);
    OBTE_REQUIRE_ALIGNED(who, score_out, "score_out", 4);
    OBTE_REQUIRE_ALIGNED(who, parent, "parent", 4);
    OBTE_REQUIRE_ALIGNED(who, ancestry_in, "ancestry_in", 4);
    OBTE_REQUIRE_ALIGNED(who, ancestry_out, "ancestry_out", 4);
    OBTE_REQUIRE_ALIGNED(who, token, "token", 8);
    OBTE_REQUIRE_ALIGNED(who, token_hist, "token_hist", 8);
    const int64_t B = P * W;
    OBTE_REQUIRE(!overlap(ancestry_in, ancestry_out, B * T_suf * 4), "%s: ancestry_in and ancestry_out must not overlap", who);
    const int64_t need = obte_beam_select_ws_bytes(P, W);
    OBTE_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0, "%s: a 16-byte aligned workspace of %lld bytes is needed, got %lld", who, (long long)need,
                 (long long)(ws ? ws_bytes : 0));

    hipStream_t st = (hipStream_t)s;
    BeamRowParams rp;
    rp.logits = (const bf16*)logits; rp.ld = ld; rp.score_in = score_in; rp.done_in = done_in; rp.allowed = allowed; rp.allowed_ld = allowed_ld;
    rp.cand = (uint32_t*)ws; rp.stat = (RowStat*)((char*)ws + cand_bytes(B, W)); rp.V = (int32_t)V; rp.W = (int32_t)W;
    int prof = obte_prof_begin(st, 116, B, V, W);
    const dim3 grid((unsigned)B);
    if (V <= 256 * 8) hipLaunchKernelGGL((beam_rows_kernel<256, 1>), grid, dim3(256), 0, st, rp);
    else if (V <= 1024 * 8 * 2) hipLaunchKernelGGL((beam_rows_kernel<1024, 2>), grid, dim3(1024), 0, st, rp);
    else hipLaunchKernelGGL((beam_rows_kernel<1024, 8>), grid, dim3(1024), 0, st, rp);
    obte_prof_end(prof, st);

    BeamMergeParams mp;
    mp.cand = rp.cand; mp.stat = rp.stat; mp.anc_in = ancestry_in; mp.anc_out = ancestry_out; mp.parent = parent; mp.token = token;
    mp.score_out = score_out; mp.done_out = done_out; mp.token_row = token_hist + slot * B; mp.T_suf = T_suf;
    mp.W = (int32_t)W; mp.slot = (int32_t)slot; mp.eos = (int32_t)eos_token;
    prof = obte_prof_begin(st, 117, P, W, slot);
    const dim3 mgrid((unsigned)P);
    if (W * W <= 64) hipLaunchKernelGGL((beam_merge_kernel<64>), mgrid, dim3(64), 0, st, mp);
    else if (W * W <= 256) hipLaunchKernelGGL((beam_merge_kernel<256>), mgrid, dim3(256), 0, st, mp);
    else hipLaunchKernelGGL((beam_merge_kernel<1024>), mgrid, dim3(1024), 0, st, mp);
    obte_prof_end(prof, st);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}
