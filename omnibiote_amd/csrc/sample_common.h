// What the kernels that turn a row of bf16 logits into a distribution share (sample.hip: the draw; spec_verify.hip: draft verification):
// the row as order-preserving 16-bit keys in registers, its maximum, the two-level select of the top-k / top-p threshold and the 2^40
// fixed-point weights.  Every sum is an integer sum, so what one kernel computes of a row — threshold, kept count, total, an entry's
// weight — is bit for bit what the other computes, whatever the workgroup shape.
//   load     16 bytes per lane, wave w owning the contiguous chunks [w R 64, (w + 1) R 64) of 8 columns (chunk (w R + j) 64 + lane in
//            register group j: coalesced per wave and in index order wave by wave).  Columns >= V, NaN and -inf become key 0 = "never kept",
//            and so do the columns a restriction excludes (sp_load_row_masked: one mask byte per chunk, an AND before the fence).
//   maximum  one u32 max over key << 16 | (65535 - column): the row maximum and, among its ties, the lowest column.
//   select   "the first value, walking the distinct values downwards, at which the running sum reaches a target": top-k with weight 1
//            and target k, top-p with the fixed-point weights and target ceil(top_p total).  Two levels: 4096 bins of the key's upper 12
//            bits (the upper byte alone is sign and exponent: a row of logits lands in a handful of its values and the LDS atomics would
//            queue up behind each other), then 16 bins of the lower 4 bits inside the chosen bin.  The sums are integers: the result does
//            not depend on the order the atomics arrive in.
// Weights: w = floor(exp2((x - max) log2(e) / T) 2^40), the maximum's own weight 2^40 exactly; 65 536 of them sum below 2^57.
#pragma once
#include "common.h"
#include <math.h>

namespace {

typedef unsigned long long u64;
constexpr int SP_BINS = 4096;
constexpr u64 SP_ONE = 1ull << 40;
constexpr int SP_MAX_V = 65536;

// bf16 bits -> key: a > b as values <=> key(a) > key(b); -0 counts as +0; 0 = NaN or -inf (every other key is >= 0x0080)
__device__ __forceinline__ uint32_t sp_key(uint32_t b) {
    b = b == 0x8000u ? 0u : b;
    const uint32_t k = (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
    return ((b & 0x7FFFu) > 0x7F80u || b == 0xFF80u) ? 0u : k;
}
__device__ __forceinline__ float sp_val(uint32_t k) {
    const uint32_t b = (k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xFFFFu);
    return __builtin_bit_cast(float, b << 16);
}
__device__ __forceinline__ u64 sp_weight(uint32_t key, uint32_t maxkey, float maxv, float scale) {
    if (key == maxkey) return SP_ONE;   // (also the +inf row: inf - inf is never formed)
    const float f = __builtin_amdgcn_exp2f((sp_val(key) - maxv) * scale) * 0x1p40f;
    return (u64)fminf(f, 0x1p40f);
}

// The 8 columns of chunk c of the row x as 4 registers of two keys each, columns >= V as key 0.  The group holding column V - 1 is read
// whole: ld >= 8 nch keeps it inside the row.
__device__ __forceinline__ void sp_load_chunk(const bf16* x, int c, int nch, int V, uint32_t (&k)[4]) {
    u32x4 raw = {0u, 0u, 0u, 0u};
    if (c < nch) raw = *reinterpret_cast<const u32x4*>(x + (int64_t)c * 8);
    const int nv = V - c * 8;   // columns of this group inside the row (<= 0: none)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t lo = 2 * q < nv ? sp_key(raw[q] & 0xFFFFu) : 0u;
        const uint32_t hi = 2 * q + 1 < nv ? sp_key(raw[q] >> 16) : 0u;
        k[q] = lo | (hi << 16);
    }
}

// the thread's 8 R columns of the row: register group j holds chunk chunk0 + 64 j
template <int R>
__device__ __forceinline__ void sp_load_row(const bf16* x, int chunk0, int V, uint32_t (&k)[R][4]) {
    const int nch = (V + 7) >> 3;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        sp_load_chunk(x, chunk0 + j * 64, nch, V, k[j]);
#pragma unroll
        for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(k[j][q]));   // opaque: 32 packed registers stay 32, the passes unpack as they go
    }
}

// ---- a restricted row (include/omnibiote_hip_constrain.h): excluded columns become key 0 at load time, nothing after the load changes ----
struct SpConstraint {          // a call's restriction, as the host hands it over (allowed NULL: no mask; hold_token -1: nothing held)
    const uint8_t* allowed;
    int64_t allowed_ld;        // bytes between the rows' masks, 0: one mask for every row
    const int32_t* emitted;
    int32_t hold_token;        // already inside [0, V), or -1
    int32_t min_emitted;
};
struct SpRowMask {             // one logits row's share of it
    const uint8_t* bits;       // ceil(V / 8) bytes, or NULL
    int hold;                  // the column held in this row, or -1
};
// batch row b at drafted position j (0 in the sampler): the hold applies while emitted[b] + j < min_emitted, summed in 64 bits
__device__ __forceinline__ SpRowMask sp_row_mask(const SpConstraint& c, int64_t b, int j) {
    SpRowMask m;
    m.bits = c.allowed ? c.allowed + b * c.allowed_ld : nullptr;
    m.hold = -1;
    if (c.hold_token >= 0) {
        const int64_t e = c.emitted ? (int64_t)c.emitted[b] : 0;
        if (e + j < (int64_t)c.min_emitted) m.hold = c.hold_token;
    }
    return m;
}
// the 8 bits of chunk c's columns, a clear bit = excluded (bits of columns >= V mean nothing: sp_load_chunk has made those keys 0)
__device__ __forceinline__ uint32_t sp_mask_byte(const SpRowMask& m, int c, int nch) {
    uint32_t bits = 0xFFu;
    if (m.bits && c < nch) bits = m.bits[c];
    if ((m.hold >> 3) == c) bits &= ~(1u << (m.hold & 7));   // (hold = -1: chunk -1, never)
    return bits;
}
// sp_load_chunk under such a byte: the bits take the place of the test "column < V" (a bit field extract and an AND per key where the
// plain load has a compare and a select), so a restricted row costs the plain load's instructions plus a few per chunk.  The packing
// is a function of its own: the penalised load rewrites the 16 bytes between the load and it.
__device__ __forceinline__ void sp_pack_chunk_masked(const u32x4& raw, int c, int V, uint32_t bits, uint32_t (&k)[4]) {
    const int nv = V - c * 8;   // columns of this group inside the row (<= 0: none)
    const uint32_t in = bits & (nv >= 8 ? 0xFFu : nv <= 0 ? 0u : (1u << nv) - 1u);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t lo = sp_key(raw[q] & 0xFFFFu) & (uint32_t)(-(int32_t)((in >> (2 * q)) & 1u));
        const uint32_t hi = sp_key(raw[q] >> 16) & (uint32_t)(-(int32_t)((in >> (2 * q + 1)) & 1u));
        k[q] = lo | (hi << 16);
    }
}
__device__ __forceinline__ void sp_load_chunk_masked(const bf16* x, int c, int nch, int V, uint32_t bits, uint32_t (&k)[4]) {
    u32x4 raw = {0u, 0u, 0u, 0u};
    if (c < nch) raw = *reinterpret_cast<const u32x4*>(x + (int64_t)c * 8);
    sp_pack_chunk_masked(raw, c, V, bits, k);
}
// is column t (inside [0, V)) of the row excluded?
__device__ __forceinline__ bool sp_excluded(const SpRowMask& m, int t) {
    return t == m.hold || (m.bits && !((m.bits[t >> 3] >> (t & 7)) & 1u));
}

// the host's checks of a restriction (OBTE_EINVAL before any launch); `out` is what the kernels get: hold_token inside [0, V) or -1
inline int sp_check_constraint(const char* who, const SpConstraint& c, int64_t hold_token, int64_t V, SpConstraint* out) {
    OBTE_REQUIRE(c.allowed_ld >= 0, "%s: allowed_ld must not be negative, got %lld", who, (long long)c.allowed_ld);
    OBTE_REQUIRE(c.allowed_ld == 0 || c.allowed_ld >= (V + 7) / 8, "%s: allowed_ld %lld is smaller than the ceil(V / 8) = %lld bytes of a mask row", who,
                 (long long)c.allowed_ld, (long long)((V + 7) / 8));
    OBTE_REQUIRE_ALIGNED(who, c.emitted, "emitted", 4);
    OBTE_REQUIRE(c.min_emitted >= 0, "%s: min_emitted must not be negative, got %d", who, (int)c.min_emitted);
    *out = c;
    out->hold_token = hold_token >= 0 && hold_token < V ? (int32_t)hold_token : -1;
    return OBTE_OK;
}

// sp_load_row of a restricted row: the lane that loads chunk c loads byte c of the row's mask — 64 consecutive bytes per wave and
// register group — and clears the excluded keys before the fence.  The R mask bytes are fetched first, all in flight at once and
// without a branch (the index is clamped: a chunk >= nch holds key 0 whatever its byte says), so that the row's own loads, which
// follow one another, wait for one more memory latency and not for R more.
template <int R>
__device__ __forceinline__ void sp_load_row_masked(const bf16* x, int chunk0, int V, const SpRowMask& m, uint32_t (&k)[R][4]) {
    const int nch = (V + 7) >> 3;
    uint32_t bits[R];
#pragma unroll
    for (int j = 0; j < R; ++j) bits[j] = 0xFFu;
    if (m.bits) {
#pragma unroll
        for (int j = 0; j < R; ++j) bits[j] = m.bits[min(chunk0 + j * 64, nch - 1)];
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int c = chunk0 + j * 64;
        if ((m.hold >> 3) == c) bits[j] &= ~(1u << (m.hold & 7));   // (hold = -1: chunk -1, never)
        sp_load_chunk_masked(x, c, nch, V, bits[j], k[j]);
#pragma unroll
        for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(k[j][q]));
    }
}

// ---- a penalised row (include/omnibiote_hip_penalty.h): the columns of the row's history are rewritten at load time, nothing after the
// load changes.  The workgroup first counts the history into a table in LDS, one 16-bit entry per column (two per 32-bit word): bit 15
// = "in the prompt", bits 0..14 = how often the column was generated (<= gen_max <= 32767: a count never reaches bit 15).  The sums
// are integers, so the table does not depend on the order the LDS atomics arrive in.
struct SpPenalty {             // a call's penalties, as the host hands them over (a NULL list has the bound 0)
    const int64_t* prompt;
    int64_t prompt_ld;
    const int32_t* prompt_len; // or NULL: every row holds prompt_max
    const int64_t* gen;
    int64_t gen_ld;
    const int32_t* n_gen;      // or NULL: 0
    int64_t n_gen_all;
    int32_t prompt_max, gen_max;
    float repetition, inv_repetition, presence, frequency;
};
// clamp(n + add, 0, hi), the sum in 64 bits: it cannot overflow, whatever the count holds
__device__ __forceinline__ int sp_count(const int32_t* n, int64_t b, int64_t add, int32_t hi) {
    const int64_t v = (n ? (int64_t)n[b] : 0) + add;
    return (int)(v < 0 ? 0 : v > (int64_t)hi ? (int64_t)hi : v);
}
// Row b's history into `table` (16 nch bytes, 16-byte aligned): cleared, a barrier, the two lists walked NT entries at a time (ids outside
// [0, V) are skipped: no index is formed from them), a barrier.  Exactly the row's prompt_len_b and n_gen_b entries are read.
template <int NT>
__device__ __forceinline__ void sp_history_table(const SpPenalty& pen, int64_t b, int V, uint32_t* table) {
    const int tid = threadIdx.x, nch = (V + 7) >> 3;
    const int np = pen.prompt_max > 0 ? sp_count(pen.prompt_len, b, pen.prompt_len ? 0 : pen.prompt_max, pen.prompt_max) : 0;
    const int ng = pen.gen_max > 0 ? sp_count(pen.n_gen, b, pen.n_gen_all, pen.gen_max) : 0;
    const int64_t* prompt = pen.prompt + b * pen.prompt_ld;
    const int64_t* gen = pen.gen + b * pen.gen_ld;
    // the first NT ids of both lists are fetched ahead of the clear: one memory round trip under it instead of two behind it
    int64_t tp = tid < np ? prompt[tid] : -1, tg = tid < ng ? gen[tid] : -1;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int c = tid; c < nch; c += NT) reinterpret_cast<u32x4*>(table)[c] = zero;
    __syncthreads();
    for (int i = tid; i < np; i += NT) {
        if (i != tid) tp = prompt[i];
        if ((u64)tp < (u64)V) atomicOr(&table[tp >> 1], 0x8000u << (16 * ((int)tp & 1)));
    }
    for (int i = tid; i < ng; i += NT) {
        if (i != tid) tg = gen[i];
        if ((u64)tg < (u64)V) atomicAdd(&table[tg >> 1], 1u << (16 * ((int)tg & 1)));
    }
    __syncthreads();
}
// the bf16 bits b of a column whose table entry e is not 0, penalised: every operation rounded to fp32 on its own, then to bf16 (nearest even)
__device__ __forceinline__ uint32_t sp_penalize(uint32_t b, uint32_t e, const SpPenalty& pen) {
#pragma clang fp contract(off)
    float x = __builtin_bit_cast(float, b << 16);
    if (pen.repetition != 1.0f) x = x < 0.0f ? x * pen.repetition : x * pen.inv_repetition;
    const uint32_t c = e & 0x7FFFu;
    if (c) {
        const float prod = pen.frequency * (float)c;
        const float sum = pen.presence + prod;
        x = x - sum;
    }
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    return x != x ? 0x7FC0u : (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
// sp_load_row_masked of a penalised row: the lane that loads chunk c reads the chunk's eight entries as one 16-byte LDS read and rewrites
// the bits of the columns whose entry is not 0 before it packs the keys.  The row's own loads and the mask bytes are issued ahead of
// the table's two barriers, so their latency passes under the history's.
template <int NT, int R>
__device__ __forceinline__ void sp_load_row_penalized(const bf16* x, int chunk0, int V, const SpRowMask& m, const SpPenalty& pen, int64_t b, uint32_t* table,
                                                      uint32_t (&k)[R][4]) {
    const int nch = (V + 7) >> 3;
    uint32_t bits[R];
    u32x4 raw[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int c = chunk0 + j * 64;
        bits[j] = m.bits ? (uint32_t)m.bits[min(c, nch - 1)] : 0xFFu;
        const u32x4 zero = {0u, 0u, 0u, 0u};
        raw[j] = c < nch ? *reinterpret_cast<const u32x4*>(x + (int64_t)c * 8) : zero;
    }
    sp_history_table<NT>(pen, b, V, table);
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int c = chunk0 + j * 64;
        if (c < nch) {
            const u32x4 e = reinterpret_cast<const u32x4*>(table)[c];
            if (e[0] | e[1] | e[2] | e[3]) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    uint32_t lo = raw[j][q] & 0xFFFFu, hi = raw[j][q] >> 16;
                    if (e[q] & 0xFFFFu) lo = sp_penalize(lo, e[q] & 0xFFFFu, pen);
                    if (e[q] >> 16) hi = sp_penalize(hi, e[q] >> 16, pen);
                    raw[j][q] = lo | (hi << 16);
                }
            }
        }
        if ((m.hold >> 3) == c) bits[j] &= ~(1u << (m.hold & 7));   // (hold = -1: chunk -1, never)
        sp_pack_chunk_masked(raw[j], c, V, bits[j], k[j]);
#pragma unroll
        for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(k[j][q]));
    }
}

// f(key, slot) over the thread's 8 R entries, slot = 8 j + i a compile-time constant that rises with the column; everything indexes k
// statically (the keys stay in registers)
template <int R, typename F>
__device__ __forceinline__ void sp_each(const uint32_t (&k)[R][4], F f) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f(k[j][q] & 0xFFFFu, 8 * j + 2 * q);
            f(k[j][q] >> 16, 8 * j + 2 * q + 1);
        }
        __builtin_amdgcn_sched_barrier(0);   // one group of 8 at a time: interleaving the groups' temporaries costs registers the keys need
    }
}

template <int NT>
__device__ __forceinline__ uint32_t sp_block_max(uint32_t v, u64* red) {
    constexpr int NW = NT / 64;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    __syncthreads();   // red is free again
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t r = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) r = max(r, (uint32_t)red[w]);
    return r;
}

// maximum key << 16 | (65535 - its lowest column) over the row (0: no entry above -inf that is not NaN)
template <int NT, int R>
__device__ __forceinline__ uint32_t sp_row_max(const uint32_t (&k)[R][4], int chunk0, u64* red) {
    uint32_t best = 0;   // the thread's largest key and, among its ties, the lowest slot = the lowest column
    sp_each<R>(k, [&](uint32_t key, int slot) { best = max(best, (key << 16) | (uint32_t)(8 * R - 1 - slot)); });
    {
        const int slot = 8 * R - 1 - (int)(best & 0xFFFFu);
        const int e = (chunk0 + (slot >> 3) * 64) * 8 + (slot & 7);
        best = (best >> 16) ? (best & 0xFFFF0000u) | (uint32_t)(65535 - e) : 0u;
    }
    return sp_block_max<NT>(best, red);
}

__device__ __forceinline__ u64 sp_wave_scan(u64 v) {   // inclusive
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
// exclusive prefix of v over the workgroup in thread order, and the total
template <int NT>
__device__ __forceinline__ u64 sp_block_scan(u64 v, u64* red, u64& total) {
    constexpr int NW = NT / 64;
    const int wave = threadIdx.x >> 6;
    const u64 inc = sp_wave_scan(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 63) red[wave] = inc;
    __syncthreads();
    u64 base = 0, tot = 0;
#pragma unroll 2
    for (int w = 0; w < NW; ++w) {
        const u64 r = red[w];
        base += w < wave ? r : 0;
        tot += r;
    }
    total = tot;
    return base + inc - v;
}

// The largest key t with sum over {thr <= key, t <= key} of weight >= target (MASS: the fixed-point weights, target = ceil(frac total);
// otherwise weight 1, target = count).  Fewer entries than the target: thr comes back (no cut).
template <int NT, int R, bool MASS>
__device__ __forceinline__ uint32_t sp_select(const uint32_t (&k)[R][4], uint32_t thr, uint32_t maxkey, float maxv, float scale, u64 count,
                                              float frac, u64* hist, u64* hist2, u64* red, u64* sel) {
    constexpr int BPT = SP_BINS / NT;
    const int tid = threadIdx.x;
    __syncthreads();   // nobody still reads hist2 / sel of an earlier select
    for (int i = tid; i < SP_BINS; i += NT) hist[i] = 0;
    if (tid < 16) hist2[tid] = 0;
    if (tid == 0) { sel[0] = ~0ull; sel[1] = 0; }
    __syncthreads();
    sp_each<R>(k, [&](uint32_t key, int) {
        if (key >= thr) {
            const u64 w = MASS ? sp_weight(key, maxkey, maxv, scale) : 1ull;
            if (w) atomicAdd(&hist[key >> 4], w);
        }
    });
    __syncthreads();
    u64 tsum = 0;   // this thread's BPT bins, the highest first
#pragma unroll
    for (int i = 0; i < BPT; ++i) tsum += hist[SP_BINS - 1 - (tid * BPT + i)];
    u64 total;
    const u64 excl = sp_block_scan<NT>(tsum, red, total);
    u64 target = count;
    if (MASS) {
        const double t = ceil((double)frac * (double)total);
        target = t < 1.0 ? 1ull : (u64)t;
        target = target > total ? total : target;
    }
    if (excl < target && target <= excl + tsum) {   // at most one thread
        u64 cum = excl, before = 0;
        int found = -1;
#pragma unroll
        for (int i = 0; i < BPT; ++i) {
            const int bin = SP_BINS - 1 - (tid * BPT + i);
            const u64 h = hist[bin];
            if (found < 0 && cum + h >= target) { found = bin; before = cum; }
            cum += h;
        }
        sel[0] = (u64)found;
        sel[1] = before;
    }
    __syncthreads();
    const u64 sbin = sel[0];
    if (sbin == ~0ull) return thr;
    sp_each<R>(k, [&](uint32_t key, int) {
        if (key >= thr && (key >> 4) == (uint32_t)sbin) {
            const u64 w = MASS ? sp_weight(key, maxkey, maxv, scale) : 1ull;
            if (w) atomicAdd(&hist2[key & 15u], w);
        }
    });
    __syncthreads();
    u64 cum = sel[1];
    uint32_t res = (uint32_t)sbin << 4;
    bool done = false;
#pragma unroll 2
    for (int d = 15; d >= 0; --d) {
        const u64 h = hist2[d];
        if (!done && cum + h >= target) { res = ((uint32_t)sbin << 4) | (uint32_t)d; done = true; }
        cum += h;
    }
    return max(res, thr);
}

// The threshold key of the row's kept set: top-k on everything valid, then top-p on what top-k kept (1: no cut)
template <int NT, int R>
__device__ __forceinline__ uint32_t sp_threshold(const uint32_t (&k)[R][4], uint32_t maxkey, float maxv, float scale, int V, int top_k, float top_p,
                                                 u64* hist, u64* hist2, u64* red, u64* sel) {
    uint32_t thr = 1;
    if (top_k > 0 && top_k < V) thr = sp_select<NT, R, false>(k, thr, maxkey, maxv, scale, (u64)top_k, 0.f, hist, hist2, red, sel);
    if (top_p < 1.0f) thr = sp_select<NT, R, true>(k, thr, maxkey, maxv, scale, 0, top_p, hist, hist2, red, sel);
    return thr;
}

// The draw's target in the integer distribution of `total`: the token is the first entry, in index order, whose running sum exceeds it
// (u >= 1: the last entry of non-zero weight; u < 0 or NaN: the first)
__device__ __forceinline__ u64 sp_draw_target(float u, u64 total) {
    u64 target = 0;
    if (u >= 1.0f) target = total - 1;
    else if (u > 0.0f) {
        target = (u64)((double)u * (double)total);
        target = target > total - 1 ? total - 1 : target;
    }
    return target;
}

// the thread's kept mass and kept count, summed over the workgroup: (this wave's base in wave order, the wave's own sum in `mass`, the
// row's total, the row's kept count)
template <int NT, int R>
__device__ __forceinline__ void sp_row_mass(const uint32_t (&k)[R][4], uint32_t thr, uint32_t maxkey, float maxv, float scale, u64* red, u64* red_n,
                                            u64& mass, u64& base, u64& total, u64& n) {
    constexpr int NW = NT / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 cnt = 0;
    mass = 0;
    sp_each<R>(k, [&](uint32_t key, int) {
        if (key >= thr) { mass += sp_weight(key, maxkey, maxv, scale); cnt += 1; }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mass += __shfl_xor(mass, o, 64); cnt += __shfl_xor(cnt, o, 64); }
    __syncthreads();
    if (lane == 0) { red[wave] = mass; red_n[wave] = cnt; }
    __syncthreads();
    base = 0; total = 0; n = 0;
#pragma unroll 2
    for (int w = 0; w < NW; ++w) {
        const u64 r = red[w];
        base += w < wave ? r : 0;
        total += r;
        n += red_n[w];
    }
}

}  // namespace
