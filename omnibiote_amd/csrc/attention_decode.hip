// Autoregressive generation: the key/value cache and attention for ONE query per (batch, head) (include/omnibiote_hip.h,
// "autoregressive generation"; extends training/model.py:115-130, whose generate() the reference struck out).
//
// One layer's cache comes in four formats, and every kernel of this file is written once over a format struct (CacheBf16, CacheE4m3, CachePaged,
// CachePaged8):
//   - bf16 (include/omnibiote_hip.h): K [B, H, T_max, hs] followed by V in the same shape: a (b, h)'s keys are hs * 2 bytes apart, so a
//     step streams them as one contiguous run.
//   - OCP e4m3 (include/omnibiote_hip_kv8.h; the format in words and in plain torch: omnibiote_amd/kvquant.py): K codes uint8
//     [B, H, T_max, hs], V codes in the same shape, K scales fp32 [B, H, T_max], V scales: 2 (hs + 4) bytes per (b, h, position) against
//     4 hs.  A head vector x of hs bf16 values is stored as code_i = RNE_e4m3(x_i 2^-e) and scale = 2^e, e the smallest integer >= -126
//     with max|x_i| 2^-e <= 448: a power of two, so the product is exact, the only rounding is the conversion's, nothing saturates, and
//     the cache is a pure function of the bf16 inputs.
//   - bf16 in pages (include/omnibiote_hip_paged.h; in plain torch: omnibiote_amd/paged.py): K [n_pages, H, 64, hs] followed by V, and an
//     int32 table [rows, table_ld] that says which page holds positions [64 j, 64 j + 64) of row b: the same vectors at other addresses.
//   - e4m3 in pages (include/omnibiote_hip_paged8.h): K codes [n_pages, H, 64, hs], V codes, K scales fp32 [n_pages, H, 64], V scales, under
//     the same table: the e4m3 cache's codes and scales at other addresses.
// A format states what differs: the dims a lane holds (DPL), where V and the scales lie behind K, how a lane's piece of a key is loaded
// and turned into floats, whether a per-key scale exists, and how 8 values of a head vector are written to the cache.
//
// The store (kv_store_kernel) copies the k and v thirds of a packed qkv activation there, one thread per 16 bytes of qkv; its ROPE form
// (the rows forms below) rotates the q and k thirds in place first.
//
// The attention (attn_decode_kernel) is bound by the read of the cache (bf16: 4 hs bytes per key against 4 hs flops).  No MFMA, no LDS staging:
//   - grid (split, b H + h); a workgroup of 4 waves owns the keys [k0, k1) of its split.  hs / DPL lanes share one key, each holding DPL
//     dims of its K row and of its V row (bf16: 16 bytes, a wave's load instruction covers 1 KiB of consecutive rows), and the lane that
//     multiplies dims DPL c .. DPL c + DPL - 1 of q by K is the one that accumulates those dims of P V.  UNROLL keys per lane group are
//     loaded (K and V: 2 UNROLL loads in flight per lane) before the first of them is used.
//   - q sits in DPL fp32 registers per lane with scale * log2(e) folded in; a score is DPL FMAs and a DPP sum over the key's lanes.  Every
//     lane group runs its own online softmax (m, l, acc[DPL] in fp32, exp2 domain): nothing crosses lanes inside the loop but the score.
//     e4m3: the key's scale multiplies the score after the group sum, the value's scale the probability used for P V, l sums the
//     unscaled probability.
//   - the groups of a wave merge by lane exchange, the waves through LDS in wave order; the workgroup writes o / lse itself (one split)
//     or an fp32 partial (acc[hs], m, l) to the workspace, which a second launch combines in split order.  No atomics, no flags.
//   - a key at or beyond k1 never enters: its loads (e4m3: its scale loads too) are redirected to the split's last key, its score is
//     -inf, its weight an exact 0 and its V a selected 0, so whatever the cache holds past n_keys (NaN patterns included) cannot reach
//     the result.  A lane group, a wave or a split without any key carries (m = -inf, l = 0, acc = 0); every merge rescales against a
//     maximum made finite first, so exp2(-inf - -inf) is never formed.
//
// The rows forms (obte_kv_cache_rope_store_rows and its n-positions form obte_kv_cache_rope_store_chunk, obte_kv8_cache_rope_store_rows;
// obte_attn_decode_rows, obte_attn_decode_kv8 with n_keys_rows): one position / key count PER ROW, an int32 the kernels read on the device,
// for a batch whose rows stand at different positions.  A value outside the host's bound makes the row inactive: nothing of it is stored,
// none of its cache is read, its attention output is exact zeros and its lse -inf — an out-of-range device value is memory-safe without
// a status word, and a negative one parks a finished row.  The attention kernel is the one above with ROWS = true: a workgroup derives
// its key range from its own row's count by the host's formula, so a row of n keys under s splits is partitioned (and summed) exactly
// as obte_attn_decode partitions n keys under s splits.
#include "common.h"

#ifndef KV8_DPL
#define KV8_DPL 16   // e4m3: 8 or 16 dims (= code bytes) per lane and key (DESIGN.md 14.7 has both register reports and the measurement that chose)
#endif

namespace {

constexpr int DEC_WAVES = 4;     // waves per workgroup
constexpr int DEC_UNROLL = 4;    // keys per lane group whose loads are in flight together (bf16 cache: K and V, 8 loads of 16 bytes per lane)
constexpr int DEC_CHUNK = 64;    // split boundaries are multiples of this many keys (16 KiB of K at head size 128 in bf16)
// (DEC_PAD: common.h — attention_shared.hip reads the partials)

// OP over every aligned group of LPR (4, 8 or 16) consecutive lanes, the result on each lane of the group
template <int LPR, bool MAX>
__device__ __forceinline__ float group_reduce(float v) {
    auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : a + b; };
    v = op(v, dpp_moved<0xB1>(v));                        // quad_perm [1,0,3,2]
    v = op(v, dpp_moved<0x4E>(v));                        // quad_perm [2,3,0,1]
    if (LPR >= 8) v = op(v, dpp_moved<0x141>(v));         // row_half_mirror: 8 lanes
    if (LPR == 16) v = op(v, dpp_moved<0x140>(v));        // row_mirror: 16 lanes
    return v;
}

// ---- the two cache formats ------------------------------------------------------------------------------------------------------------------
// Both are built from the cache pointer and n_vec = B H T_max, the head vectors of K.  The attention's view: the (b, h) = bh's K and V rows
// (k, v; SCALED: the scale rows ks, vs), load(ptr): a lane's Piece of a key's row, DPL elements at ptr, to_float: its DPL values.
// The store's view: put(which, vec, hs, e, x): the 8 values x at dims e .. e + 7 of head vector vec of K (which = 0) or V (1), called
// by all hs / 8 consecutive lanes of a head vector at once.

struct CacheBf16 {
    static constexpr bool ANC = false;
    static constexpr bool PAGED = false;
    static constexpr int DPL = 8;
    static constexpr bool SCALED = false;
    typedef u32x4 Piece;
    bf16 *k, *v;
    __device__ __forceinline__ CacheBf16(void* cache, int64_t n_vec, int hs, int64_t bh = 0, int64_t T_max = 0)
        : k((bf16*)cache + bh * T_max * hs), v(k + n_vec * hs) {}
    static __device__ __forceinline__ Piece load(const bf16* p) { return *(const u32x4*)p; }
    static __device__ __forceinline__ void to_float(Piece r, float* f) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f[2 * j] = __builtin_bit_cast(float, r[j] << 16);
            f[2 * j + 1] = __builtin_bit_cast(float, r[j] & 0xFFFF0000u);
        }
    }
    __device__ __forceinline__ void put(int which, int64_t vec, int hs, int e, bf16x8 x) const { *(bf16x8*)((which ? v : k) + vec * hs + e) = x; }
};

// the bf16 cache read through an ancestry table (include/omnibiote_hip_beam.h): the same bytes, another row per key
struct CacheBf16Anc : CacheBf16 {
    static constexpr bool ANC = true;
    using CacheBf16::CacheBf16;
};

// the bf16 vectors in a pool of pages (include/omnibiote_hip_paged.h): K [n_pages, H, 64, hs], V behind it; n_vec = n_pages H 64.  The
// attention's view: k and v are head h's block of page 0, a page is H 64 hs elements further; the store's view: vec = (page H + h) 64 + slot
struct CachePaged : CacheBf16 {
    static constexpr bool PAGED = true;
    using CacheBf16::CacheBf16;
};

struct CacheE4m3 {
    static constexpr bool ANC = false;
    static constexpr bool PAGED = false;
    static constexpr int DPL = KV8_DPL;
    static constexpr bool SCALED = true;
    typedef __attribute__((ext_vector_type(DPL / 4))) uint32_t Piece;   // DPL code bytes
    uint8_t *k, *v;
    float *ks, *vs;
    __device__ __forceinline__ CacheE4m3(void* cache, int64_t n_vec, int hs, int64_t bh = 0, int64_t T_max = 0)
        : k((uint8_t*)cache + bh * T_max * hs), v(k + n_vec * hs), ks((float*)((uint8_t*)cache + 2 * n_vec * hs) + bh * T_max), vs(ks + n_vec) {}
    static __device__ __forceinline__ Piece load(const uint8_t* p) { return *(const Piece*)p; }
    static __device__ __forceinline__ void to_float(Piece w, float* f) {   // v_cvt_pk_f32_fp8: two of a word's four bytes at a time
        typedef __attribute__((ext_vector_type(2))) float f32x2;
#pragma unroll
        for (int j = 0; j < DPL / 4; ++j) {
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
            f[4 * j] = lo[0]; f[4 * j + 1] = lo[1]; f[4 * j + 2] = hi[0]; f[4 * j + 3] = hi[1];
        }
    }
    // the maximum over the vector's lanes by DPP, the exponent from the maximum's bits in integer arithmetic, 8 codes from v_cvt_pk_fp8_f32
    // in one 8-byte store, the scale from the vector's first lane
    __device__ __forceinline__ void put(int which, int64_t vec, int hs, int e, bf16x8 x) const {
        float f[8], amax = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            f[j] = bf2f(x[j]);
            amax = fmaxf(amax, __builtin_fabsf(f[j]));
        }
        amax = hs == 128 ? group_reduce<16, true>(amax) : group_reduce<8, true>(amax);
        // amax = 1.frac 2^(ef - 127) = m 2^E with m = 1.frac / 2 in [0.5, 1) and E = ef - 126: e = E - 9 if m <= 0.875 (frac <= 0.75), else E - 8,
        // and at least -126 (what a zero or subnormal maximum gets: its ef is 0).  2^e and 2^-e are normal fp32 numbers for every finite maximum.
        const uint32_t bits = __builtin_bit_cast(uint32_t, amax);
        int ex = (int)(bits >> 23) - 135 + ((bits & 0x7FFFFFu) > 0x600000u ? 1 : 0);
        ex = ex < -126 ? -126 : ex;
        const float inv = __builtin_bit_cast(float, (uint32_t)(127 - ex) << 23);
        int w0 = 0, w1 = 0;
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0] * inv, f[1] * inv, w0, false);
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2] * inv, f[3] * inv, w0, true);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4] * inv, f[5] * inv, w1, false);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6] * inv, f[7] * inv, w1, true);
        *(u32x2*)((which ? v : k) + vec * hs + e) = u32x2{(uint32_t)w0, (uint32_t)w1};
        if (e == 0) (which ? vs : ks)[vec] = __builtin_bit_cast(float, (uint32_t)(ex + 127) << 23);
    }
};

// the e4m3 vectors in a pool of pages (include/omnibiote_hip_paged8.h): K codes [n_pages, H, 64, hs], V codes, K scales [n_pages, H, 64], V scales;
// n_vec = n_pages H 64.  The attention's view: k, v, ks and vs are head h's blocks of page 0, a page is H 64 hs codes and H 64 scales further;
// the store's view: vec = (page H + h) 64 + slot, which is where put() writes the scale as well
struct CachePaged8 : CacheE4m3 {
    static constexpr bool PAGED = true;
    using CacheE4m3::CacheE4m3;
};

// ---- the attention --------------------------------------------------------------------------------------------------------------------------
template <int DPL>
struct Part { float m, l, acc[DPL]; };   // one online-softmax state, exp2 domain: sum_k exp2(s_k - m) (1, v_k) for the DPL dims of a lane

// a += b with both rescaled to the common maximum; an empty side (m = -inf, l = 0, acc = 0) adds exactly nothing
template <int DPL>
__device__ __forceinline__ void merge(Part<DPL>& a, const Part<DPL>& b) {
    const float m = fmaxf(a.m, b.m);
    const float ms = m == -INFINITY ? 0.f : m;
    const float wa = __builtin_amdgcn_exp2f(a.m - ms), wb = __builtin_amdgcn_exp2f(b.m - ms);
    a.m = m;
    a.l = a.l * wa + b.l * wb;
#pragma unroll
    for (int j = 0; j < DPL; ++j) a.acc[j] = a.acc[j] * wa + b.acc[j] * wb;
}

// DEC_UNROLL keys of one lane group.  TAIL: some of them may lie at or beyond k1.
// ANC (the ancestry form, include/omnibiote_hip_beam.h): c is the cache of the row's GROUP (its first row, the workgroup's head), key j is
// read from the group's row anc[j], row_stride elements per row; an entry outside [0, group) is a key that is not there — as one at or
// beyond k1, with its loads sent to the group's first row.  The UNROLL entries are loaded before the first K / V load is issued.
template <class Fmt, int HS, bool TAIL, bool ANC = false>
__device__ __forceinline__ void decode_keys(Part<Fmt::DPL>& st, const float* qf, const Fmt& c, int key0, int kstride, int k1, int chunk,
                                            const int32_t* anc = nullptr, int group = 0, int64_t row_stride = 0) {
    constexpr int DPL = Fmt::DPL, LPR = HS / DPL;
    constexpr bool PAGED = Fmt::PAGED;
    typename Fmt::Piece kr[DEC_UNROLL], vr[DEC_UNROLL];
    float ksc[DEC_UNROLL], vsc[DEC_UNROLL];   // (SCALED only)
    bool ok[DEC_UNROLL];
    int from[DEC_UNROLL];                     // (ANC only; PAGED: the table entry)
    // PAGED (include/omnibiote_hip_paged.h): the round's first key is a multiple of 64, so key0 + u kstride lies in the round's page
    // u kstride / 64 for every lane; anc holds the table entries of the round's pages (the kernel fetched them a round ahead, with
    // workgroup-uniform indices; a page beyond the one of k1 - 1 is that page again: its keys are not there either way), group is the pool's
    // page count and row_stride a page's elements.  An entry outside [0, group): as in the ancestry form.
    if constexpr (PAGED) {
#pragma unroll
        for (int u = 0; u < DEC_UNROLL; ++u) from[u] = anc[u * kstride / DEC_CHUNK];
    }
    if constexpr (ANC) {
#pragma unroll
        for (int u = 0; u < DEC_UNROLL; ++u) {
            const int key = key0 + u * kstride;
            from[u] = anc[(!TAIL || key < k1) ? key : k1 - 1];
        }
    }
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
        const int key = key0 + u * kstride;
        ok[u] = !TAIL || key < k1;
        const int64_t kk = ok[u] ? key : k1 - 1;   // (k1 - 1 >= k0: a workgroup with no key never gets here)
        if constexpr (Fmt::SCALED && PAGED) {
            // Four loads per key, each a workgroup-uniform page base (a missing page: page 0, for the scales too; a page is row_stride codes
            // and row_stride / HS = H 64 scales) plus the key's slot as a 32-bit lane offset.  Written as one 64-bit offset per load the
            // address arithmetic took the registers of two of the round's sixteen loads, which then issued behind the first uses.
            // Page 0 may be a page nobody holds: what the four loads of a key that is not ok bring is dropped where it is used, below.
            const bool there = (uint32_t)from[u] < (uint32_t)group;
            ok[u] = ok[u] && there;
            const int64_t page = there ? (int64_t)from[u] : 0;
            const int slot = (int)kk & (DEC_CHUNK - 1), lo = slot * HS + chunk * DPL;
            kr[u] = Fmt::load(c.k + page * row_stride + lo);
            vr[u] = Fmt::load(c.v + page * row_stride + lo);
            ksc[u] = (c.ks + page * (row_stride / HS))[slot];
            vsc[u] = (c.vs + page * (row_stride / HS))[slot];
        } else {
            int64_t off = (PAGED ? kk & (DEC_CHUNK - 1) : kk) * HS + chunk * DPL;   // in elements, of either format; one offset for both loads: K and V addresses are formed alike
            if constexpr (ANC || PAGED) {
                const bool there = (uint32_t)from[u] < (uint32_t)group;
                ok[u] = ok[u] && there;
                off += (there ? (int64_t)from[u] : 0) * row_stride;
            }
            kr[u] = Fmt::load(c.k + off);
            vr[u] = Fmt::load(c.v + off);
            if constexpr (Fmt::SCALED) {
                ksc[u] = c.ks[kk];
                vsc[u] = c.vs[kk];
            }
        }
    }
    float sc[DEC_UNROLL];
    float mx = st.m;
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
        float kf[DPL];
        Fmt::to_float(kr[u], kf);
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < DPL; ++j) d = __builtin_fmaf(qf[j], kf[j], d);
        d = group_reduce<LPR, false>(d);
        if constexpr (Fmt::SCALED) d *= ksc[u];
        sc[u] = ok[u] ? d : -INFINITY;
        mx = fmaxf(mx, sc[u]);
    }
    const float ms = ((TAIL || ANC || PAGED) && mx == -INFINITY) ? 0.f : mx;
    const float alpha = __builtin_amdgcn_exp2f(st.m - ms);
    st.m = mx;
    st.l *= alpha;
#pragma unroll
    for (int j = 0; j < DPL; ++j) st.acc[j] *= alpha;
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
        const float p = ok[u] ? __builtin_amdgcn_exp2f(sc[u] - ms) : 0.f;
        float pv = p;
        if constexpr (Fmt::SCALED) pv = p * vsc[u];
        // a key without a page has page 0's V scale, which may be anything (a page nobody holds: NaN, Inf): 0 * NaN would reach acc.  The
        // rectangular form's key that is not ok reloads key k1 - 1, whose scale is a finite power of two: p * vsc is an exact 0 there
        if constexpr (Fmt::SCALED && PAGED) pv = ok[u] ? pv : 0.f;
        float vf[DPL];
        Fmt::to_float(ok[u] ? vr[u] : typename Fmt::Piece{}, vf);   // (a zero piece)
        st.l += p;
#pragma unroll
        for (int j = 0; j < DPL; ++j) st.acc[j] = __builtin_fmaf(pv, vf[j], st.acc[j]);
    }
}

// HS: 64 or 128.  grid (splits, B * H), DEC_WAVES * 64 threads.  per: keys per split (a multiple of DEC_CHUNK).  n_vec = B H T_max.
// splits == 1: o and lse are final.  Else part[(bh * splits + split) * (HS + DEC_PAD)] = (acc[HS], m, l).
// ROWS: row b has rows_n[b] + rows_off keys if that lies in [1, n_keys] (n_keys: the host's bound), else none (an inactive row: no
// key is loaded, the state stays (m = -inf, l = 0, acc = 0)); per is formed here from the row's own count.
// PARTIAL (the suffix part of obte_attn_decode_shared, attention_shared.hip): the state leaves as a partial at one split too, o and lse
// are not touched.
// Fmt::ANC (CacheBf16Anc, with PARTIAL and not ROWS: the suffix part of obte_attn_decode_beam): rows_n is the ancestry table [B, T_max] and
// rows_off the group size — the two arguments the uniform PARTIAL form leaves unused, so every instantiation keeps one signature and the
// instantiations behind the other entry points keep their names and their code.
template <class Fmt, int HS, bool ROWS, bool PARTIAL>
__global__ __launch_bounds__(DEC_WAVES * 64) void attn_decode_kernel(const bf16* __restrict__ q, int64_t q_ld, const void* __restrict__ cache,
                                                                      bf16* __restrict__ o, float* __restrict__ lse, float* __restrict__ part,
                                                                      int H, int64_t T_max, int64_t n_vec, int n_keys, int per, float qscale,
                                                                      const int32_t* __restrict__ rows_n, int rows_off) {
    constexpr bool ANC = Fmt::ANC;
    constexpr int DPL = Fmt::DPL;
    constexpr int LPR = HS / DPL;      // lanes per key
    constexpr int G = 64 / LPR;        // keys per wave and load
    const int split = blockIdx.x, splits = gridDim.x, bh = blockIdx.y;
    const int b = bh / H, h = bh % H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = lane % LPR, grp = lane / LPR;
    if (ROWS) {
        const int64_t n = (int64_t)rows_n[b] + rows_off;
        n_keys = (n >= 1 && n <= n_keys) ? (int)n : 0;
        per = ((n_keys + splits - 1) / splits + DEC_CHUNK - 1) / DEC_CHUNK * DEC_CHUNK;
    }
    const int k0 = min(split * per, n_keys), k1 = min(k0 + per, n_keys);

    float qf[DPL];
#pragma unroll
    for (int j = 0; j < DPL / 8; ++j) CacheBf16::to_float(*(const u32x4*)(q + b * q_ld + h * HS + chunk * DPL + j * 8), qf + j * 8);
#pragma unroll
    for (int j = 0; j < DPL; ++j) qf[j] *= qscale;

    const Fmt c(const_cast<void*>(cache), n_vec, HS, ANC ? (int64_t)(b - b % rows_off) * H + h : (int64_t)bh, T_max);   // (read only here)
    const int32_t* anc = ANC ? rows_n + (int64_t)b * T_max : nullptr;
    const int64_t row_stride = (int64_t)H * T_max * HS;   // (ANC only)
    Part<DPL> st;
    st.m = -INFINITY; st.l = 0.f;
#pragma unroll
    for (int j = 0; j < DPL; ++j) st.acc[j] = 0.f;

    constexpr int KSTRIDE = DEC_WAVES * G;              // keys between two of a lane group's UNROLL keys
    constexpr int ROUND = KSTRIDE * DEC_UNROLL;         // keys of one workgroup round
    const int full_end = k0 + (k1 - k0) / ROUND * ROUND;
    int base = k0;
    if constexpr (ANC) {
        for (; base < full_end; base += ROUND) decode_keys<Fmt, HS, false, true>(st, qf, c, base + wave * G + grp, KSTRIDE, k1, chunk, anc, rows_off, row_stride);
        if (base < k1) decode_keys<Fmt, HS, true, true>(st, qf, c, base + wave * G + grp, KSTRIDE, k1, chunk, anc, rows_off, row_stride);
    } else {
        for (; base < full_end; base += ROUND) decode_keys<Fmt, HS, false>(st, qf, c, base + wave * G + grp, KSTRIDE, k1, chunk);
        if (base < k1) decode_keys<Fmt, HS, true>(st, qf, c, base + wave * G + grp, KSTRIDE, k1, chunk);   // (workgroup-uniform)
    }

    // the lane groups of a wave: exchange with the lane LPR, 2 LPR, .. 32 away (the same dims of another key's state)
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1) {
        Part<DPL> other;
        other.m = __shfl_xor(st.m, off, 64); other.l = __shfl_xor(st.l, off, 64);
#pragma unroll
        for (int j = 0; j < DPL; ++j) other.acc[j] = __shfl_xor(st.acc[j], off, 64);
        // both partners must add in one order for the result to be the same on each: the lower lane's state first
        if (lane & off) { Part<DPL> t = other; merge(t, st); st = t; }
        else merge(st, other);
    }
    // the waves, through LDS, in wave order
    __shared__ float lds[DEC_WAVES][LPR][DPL + 2];
    if (lane < LPR) {
        lds[wave][lane][0] = st.m; lds[wave][lane][1] = st.l;
#pragma unroll
        for (int j = 0; j < DPL; ++j) lds[wave][lane][2 + j] = st.acc[j];
    }
    __syncthreads();
    if (threadIdx.x >= LPR) return;
    Part<DPL> tot;
    tot.m = lds[0][lane][0]; tot.l = lds[0][lane][1];
#pragma unroll
    for (int j = 0; j < DPL; ++j) tot.acc[j] = lds[0][lane][2 + j];
#pragma unroll
    for (int w = 1; w < DEC_WAVES; ++w) {
        Part<DPL> p;
        p.m = lds[w][lane][0]; p.l = lds[w][lane][1];
#pragma unroll
        for (int j = 0; j < DPL; ++j) p.acc[j] = lds[w][lane][2 + j];
        merge(tot, p);
    }
    if (!PARTIAL && splits == 1) {   // n_keys >= 1: l > 0; an inactive row (ROWS): l = 0, o = 0 and lse = -inf
        const float inv = (ROWS && tot.l == 0.f) ? 0.f : 1.0f / tot.l;
#pragma unroll
        for (int j = 0; j < DPL / 8; ++j) {
            bf16x8 out;
#pragma unroll
            for (int i = 0; i < 8; ++i) out[i] = f2bf(tot.acc[j * 8 + i] * inv);
            *(bf16x8*)(o + ((int64_t)bh * HS + lane * DPL + j * 8)) = out;
        }
        if (lse && lane == 0)
            lse[bh] = (ROWS && tot.l == 0.f) ? -INFINITY : (tot.m + __builtin_amdgcn_logf(tot.l)) * 0.6931471805599453f;   // v_log_f32 is log2
        return;
    }
    float* pr = part + ((int64_t)bh * splits + split) * (HS + DEC_PAD);
#pragma unroll
    for (int j = 0; j < DPL / 4; ++j) *(f32x4*)(pr + lane * DPL + j * 4) = f32x4{tot.acc[4 * j], tot.acc[4 * j + 1], tot.acc[4 * j + 2], tot.acc[4 * j + 3]};
    if (lane == 0) { pr[HS] = tot.m; pr[HS + 1] = tot.l; }
}

// The rows form over the pages of a pool (obte_attn_decode_paged, include/omnibiote_hip_paged.h): attn_decode_kernel<CacheBf16, HS, true, false>
// line for line — the same partition of a row's keys, the same rounds, merges and writes, so the same bits — with a kernel of its own only
// because it takes two more arguments, and the kernels above are to keep their argument layout and their code.  pool: K [n_pages, H, 64, hs]
// and V behind it; table [B, table_ld]: entry j of row b the page of its positions [64 j, 64 j + 64), outside [0, n_pages): no page.  Row b
// has rows_n[b] + rows_off keys if that lies in [1, max_keys] (max_keys <= 64 table_ld), else none.  k0 and ROUND are multiples of a page,
// so every round's first key is: a round's keys lie in ROUND / 64 pages known from the loop counter, and their table entries are read
// with workgroup-uniform indices (scalar loads), one round ahead: a round's K / V addresses need its entries, and a load issued at the top
// of the round would stand between every two rounds' vector loads.
// Fmt: CachePaged, or CachePaged8 (obte_attn_decode_paged8, include/omnibiote_hip_paged8.h): attn_decode_kernel<CacheE4m3, HS, true, false> in the
// same way; a round is 2 (head size 128) or 4 (64) pages, and a key's two scales come from its page's scale block.
template <class Fmt, int HS>
__global__ __launch_bounds__(DEC_WAVES * 64) void attn_decode_paged_kernel(const bf16* __restrict__ q, int64_t q_ld, const void* __restrict__ pool,
                                                                            bf16* __restrict__ o, float* __restrict__ lse, float* __restrict__ part, int H,
                                                                            int64_t table_ld, int n_pages, int max_keys, float qscale,
                                                                            const int32_t* __restrict__ rows_n, int rows_off,
                                                                            const int32_t* __restrict__ table) {
    constexpr int DPL = Fmt::DPL;
    constexpr int LPR = HS / DPL;      // lanes per key
    constexpr int G = 64 / LPR;        // keys per wave and load
    const int split = blockIdx.x, splits = gridDim.x, bh = blockIdx.y;
    const int b = bh / H, h = bh % H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = lane % LPR, grp = lane / LPR;
    const int64_t n = (int64_t)rows_n[b] + rows_off;
    const int n_keys = (n >= 1 && n <= max_keys) ? (int)n : 0;
    const int per = ((n_keys + splits - 1) / splits + DEC_CHUNK - 1) / DEC_CHUNK * DEC_CHUNK;
    const int k0 = min(split * per, n_keys), k1 = min(k0 + per, n_keys);

    float qf[DPL];
#pragma unroll
    for (int j = 0; j < DPL / 8; ++j) CacheBf16::to_float(*(const u32x4*)(q + b * q_ld + h * HS + chunk * DPL + j * 8), qf + j * 8);
#pragma unroll
    for (int j = 0; j < DPL; ++j) qf[j] *= qscale;

    const Fmt c(const_cast<void*>(pool), (int64_t)n_pages * H * DEC_CHUNK, HS, h, DEC_CHUNK);   // (read only here) head h's block of page 0
    const int32_t* row_table = table + (int64_t)b * table_ld;
    const int64_t page_stride = (int64_t)H * DEC_CHUNK * HS;
    const int last_page = (k1 - 1) / DEC_CHUNK;         // (of this split; an index beyond it is clamped to it: < table_ld by max_keys <= 64 table_ld)
    Part<DPL> st;
    st.m = -INFINITY; st.l = 0.f;
#pragma unroll
    for (int j = 0; j < DPL; ++j) st.acc[j] = 0.f;

    constexpr int KSTRIDE = DEC_WAVES * G;              // keys between two of a lane group's UNROLL keys
    constexpr int ROUND = KSTRIDE * DEC_UNROLL;         // keys of one workgroup round
    const int full_end = k0 + (k1 - k0) / ROUND * ROUND;
    int base = k0;
    static_assert(DEC_CHUNK % KSTRIDE == 0 && ROUND % DEC_CHUNK == 0, "a lane group's UNROLL keys lie in workgroup-uniform pages");
    constexpr int PAGES = ROUND / DEC_CHUNK;            // pages of one round
    int ent[PAGES], ahead[PAGES];                       // the table entries of this round's pages and of the next one's
#pragma unroll
    for (int e = 0; e < PAGES; ++e) ent[e] = k0 < k1 ? row_table[min(k0 / DEC_CHUNK + e, last_page)] : -1;
    for (; base < full_end; base += ROUND) {
#pragma unroll
        for (int e = 0; e < PAGES; ++e) ahead[e] = row_table[min((base + ROUND) / DEC_CHUNK + e, last_page)];
        decode_keys<Fmt, HS, false>(st, qf, c, base + wave * G + grp, KSTRIDE, k1, chunk, ent, n_pages, page_stride);
#pragma unroll
        for (int e = 0; e < PAGES; ++e) ent[e] = ahead[e];
    }
    if (base < k1) decode_keys<Fmt, HS, true>(st, qf, c, base + wave * G + grp, KSTRIDE, k1, chunk, ent, n_pages, page_stride);   // (workgroup-uniform)

    // the lane groups of a wave: exchange with the lane LPR, 2 LPR, .. 32 away (the same dims of another key's state)
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1) {
        Part<DPL> other;
        other.m = __shfl_xor(st.m, off, 64); other.l = __shfl_xor(st.l, off, 64);
#pragma unroll
        for (int j = 0; j < DPL; ++j) other.acc[j] = __shfl_xor(st.acc[j], off, 64);
        // both partners must add in one order for the result to be the same on each: the lower lane's state first
        if (lane & off) { Part<DPL> t = other; merge(t, st); st = t; }
        else merge(st, other);
    }
    // the waves, through LDS, in wave order
    __shared__ float lds[DEC_WAVES][LPR][DPL + 2];
    if (lane < LPR) {
        lds[wave][lane][0] = st.m; lds[wave][lane][1] = st.l;
#pragma unroll
        for (int j = 0; j < DPL; ++j) lds[wave][lane][2 + j] = st.acc[j];
    }
    __syncthreads();
    if (threadIdx.x >= LPR) return;
    Part<DPL> tot;
    tot.m = lds[0][lane][0]; tot.l = lds[0][lane][1];
#pragma unroll
    for (int j = 0; j < DPL; ++j) tot.acc[j] = lds[0][lane][2 + j];
#pragma unroll
    for (int w = 1; w < DEC_WAVES; ++w) {
        Part<DPL> p;
        p.m = lds[w][lane][0]; p.l = lds[w][lane][1];
#pragma unroll
        for (int j = 0; j < DPL; ++j) p.acc[j] = lds[w][lane][2 + j];
        merge(tot, p);
    }
    if (splits == 1) {   // n_keys >= 1: l > 0; an inactive row or one without a page: l = 0, o = 0 and lse = -inf
        const float inv = tot.l == 0.f ? 0.f : 1.0f / tot.l;
#pragma unroll
        for (int j = 0; j < DPL / 8; ++j) {
            bf16x8 out;
#pragma unroll
            for (int i = 0; i < 8; ++i) out[i] = f2bf(tot.acc[j * 8 + i] * inv);
            *(bf16x8*)(o + ((int64_t)bh * HS + lane * DPL + j * 8)) = out;
        }
        if (lse && lane == 0)
            lse[bh] = tot.l == 0.f ? -INFINITY : (tot.m + __builtin_amdgcn_logf(tot.l)) * 0.6931471805599453f;   // v_log_f32 is log2
        return;
    }
    float* pr = part + ((int64_t)bh * splits + split) * (HS + DEC_PAD);
#pragma unroll
    for (int j = 0; j < DPL / 4; ++j) *(f32x4*)(pr + lane * DPL + j * 4) = f32x4{tot.acc[4 * j], tot.acc[4 * j + 1], tot.acc[4 * j + 2], tot.acc[4 * j + 3]};
    if (lane == 0) { pr[HS] = tot.m; pr[HS + 1] = tot.l; }
}

// grid B * H, HS threads: thread d sums dim d of the partials in split order against their common maximum.  With a key in at least one
// split (n_keys >= 1) the maximum is finite and an empty split's weight is exp2(-inf) = 0.  An inactive row of the rows form has no key
// in any split: the maximum is made finite first, every weight is 0, and l = 0 gives o = 0 and lse = -inf.
template <int HS>
__global__ __launch_bounds__(HS) void attn_decode_combine_kernel(const float* __restrict__ part, bf16* __restrict__ o, float* __restrict__ lse, int splits) {
    const int bh = blockIdx.x, d = threadIdx.x;
    const float* pr = part + (int64_t)bh * splits * (HS + DEC_PAD);
    float m = -INFINITY;
    for (int s = 0; s < splits; ++s) m = fmaxf(m, pr[s * (HS + DEC_PAD) + HS]);
    const float ms = m == -INFINITY ? 0.f : m;
    float l = 0.f, acc = 0.f;
    for (int s = 0; s < splits; ++s) {
        const float* p = pr + s * (HS + DEC_PAD);
        const float w = __builtin_amdgcn_exp2f(p[HS] - ms);
        l += p[HS + 1] * w;
        acc += p[d] * w;
    }
    o[(int64_t)bh * HS + d] = f2bf(l == 0.f ? 0.f : acc / l);
    if (lse && d == 0) lse[bh] = l == 0.f ? -INFINITY : (m + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;
}

// ---- the store ------------------------------------------------------------------------------------------------------------------------------
// x rotated by (c, sn), pairwise: the arithmetic of the GEMM epilogue OBTE_EPI_ROPE_QK (fp32 on the bf16 values, the same expression: the same bits)
__device__ __forceinline__ bf16x8 rope8(bf16x8 x, f32x4 c, f32x4 sn) {
    bf16x8 rt;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float xe = bf2f(x[2 * j]), xo = bf2f(x[2 * j + 1]);
        rt[2 * j] = f2bf(xe * c[j] - xo * sn[j]);
        rt[2 * j + 1] = f2bf(xe * sn[j] + xo * c[j]);
    }
    return rt;
}

// One thread per 16 bytes of the packed qkv [B n, 3C]; a head's hs / 8 items are consecutive lanes of one wave (C / 8 and 256 are multiples
// of hs / 8), all of them in or all out.  ROPE = false: item = ((row * 2 + which) * C + column) / 8 of the k and v thirds of the rotated rows
// row = b n + j, stored at position pos0 + j.  ROPE = true (the rows form): item = ((row * 3 + third) * C + column) / 8 of the unrotated row
// b n + j at position p = pos[b] + j (0 <= pos[b] <= max_pos; any other value: the row is left alone); the q and k thirds are rotated in place
// by row p of the tables, the rotated k and the v go to cache position p of the item's head.  n = 1 is one decode step.  The ROPE entry points
// bound B n below 2^31: a row index divides in 32 bits.
// The arguments every form reads come first and fill 64 bytes: a decode step's store is a chain of argument loads, two divisions, one
// load and one store, and with the plain form's arguments spread over a second cache line (behind the tables and pos) a bf16
// decode step at 64 rows measured 0.2 - 0.3 us longer per layer.
// Fmt::PAGED (include/omnibiote_hip_paged.h): cache is the pool, n_vec = n_pages H 64, T_max the table's row length; position p of row b goes to
// slot p % 64 of page table[b][p / 64], and nowhere if that is no page of the pool (the rotation of qkv has happened by then).  table and
// n_pages stand behind every other argument: no other form reads them.
template <class Fmt, bool ROPE>
__global__ __launch_bounds__(256) void kv_store_kernel(bf16* __restrict__ qkv, void* __restrict__ cache, int64_t items, int64_t T_max, int64_t pos0,
                                                       int64_t n_vec, int n, int H, int hs, int max_pos, const float* __restrict__ cos_t,
                                                       const float* __restrict__ sin_t, const int32_t* __restrict__ pos, const int32_t* __restrict__ table,
                                                       int n_pages) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    constexpr int THIRDS = ROPE ? 3 : 2;
    const int C = H * hs, cpr = C / 8;             // 16-byte items per third of a row
    const int c8 = (int)(i % cpr);
    const int64_t rw = i / cpr;
    const int third = (int)(rw % THIRDS) + (ROPE ? 0 : 1);   // 0 q, 1 k, 2 v
    const int64_t row = rw / THIRDS;
    int64_t b, p;
    if (ROPE) {
        b = (int)row / n;
        const int p0 = pos[b];
        if (p0 < 0 || p0 > max_pos) return;
        p = (int64_t)p0 + ((int)row - (int)b * n);
    } else {
        b = row / n;
        p = pos0 + row % n;
    }
    const int col = c8 * 8, h = col / hs, e = col % hs;
    bf16* ptr = qkv + row * 3 * C + (int64_t)third * C + col;
    bf16x8 x = *(const bf16x8*)ptr;
    if (ROPE && third < 2) {
        x = rope8(x, *(const f32x4*)(cos_t + p * (hs / 2) + e / 2), *(const f32x4*)(sin_t + p * (hs / 2) + e / 2));
        *(bf16x8*)ptr = x;
    }
    if (third == 0) return;   // (uniform over a head's lanes)
    if constexpr (Fmt::PAGED) {
        const int page = table[b * T_max + p / DEC_CHUNK];
        if ((uint32_t)page >= (uint32_t)n_pages) return;   // (uniform over a head's lanes)
        Fmt(cache, n_vec, hs).put(third - 1, ((int64_t)page * H + h) * DEC_CHUNK + p % DEC_CHUNK, hs, e, x);
    } else
        Fmt(cache, n_vec, hs).put(third - 1, (b * H + h) * T_max + p, hs, e, x);
}

bool shape_ok(int64_t B, int64_t T_max, int32_t n_head, int32_t head_dim) {
    return B > 0 && B < (1ll << 31) && T_max > 0 && T_max < (1ll << 24) && n_head > 0 && n_head <= 1024 && (head_dim == 64 || head_dim == 128) &&
           B * n_head < (1ll << 31);
}

// the launch behind the five store entry points, each after its own argument checks.  pos_rows: ROPE, n positions per row from pos_rows[b]
// on (max_pos: its bound); null: n rotated positions per row from pos0 on (the kernel only reads qkv)
int kv_store_launch(const char* who, bool e4m3, const obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos_rows, int64_t max_pos,
                    int64_t B, int64_t n, int32_t n_head, int32_t head_dim, void* cache, int64_t T_max, int64_t pos0, obte_stream s) {
    const int64_t items = B * n * (pos_rows ? 3 : 2) * n_head * head_dim / 8;
    OBTE_REQUIRE(cdiv64(items, 256) < (1ll << 31), "%s: too many rows for one launch", who);
    const auto kernel = pos_rows ? (e4m3 ? kv_store_kernel<CacheE4m3, true> : kv_store_kernel<CacheBf16, true>)
                                 : (e4m3 ? kv_store_kernel<CacheE4m3, false> : kv_store_kernel<CacheBf16, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)cdiv64(items, 256)), dim3(256), 0, (hipStream_t)s, (bf16*)qkv, cache, items, T_max, pos0, B * n_head * T_max,
                       (int)n, n_head, head_dim, (int)max_pos, rope_cos, rope_sin, pos_rows, (const int32_t*)nullptr, 0);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}

// obte_kv_cache_store and obte_kv8_cache_store: the same checks
int kv_store_checked(const char* who, bool e4m3, const obte_bf16* qkv, int64_t B, int64_t t, int32_t n_head, int32_t head_dim, void* cache, int64_t T_max,
                     int64_t pos0, obte_stream s) {
    OBTE_REQUIRE(qkv && cache, "%s: null pointer", who);
    OBTE_REQUIRE(shape_ok(B, T_max, n_head, head_dim), "%s: bad shape (head_dim 64 or 128)", who);
    OBTE_REQUIRE(t > 0 && pos0 >= 0 && pos0 + t <= T_max, "%s: positions [%lld, %lld) do not fit T_max = %lld", who, (long long)pos0, (long long)(pos0 + t),
                 (long long)T_max);
    OBTE_REQUIRE((((uintptr_t)qkv | (uintptr_t)cache) & 15) == 0, "%s: qkv and cache must be 16-byte aligned", who);
    return kv_store_launch(who, e4m3, qkv, nullptr, nullptr, nullptr, 0, B, t, n_head, head_dim, cache, T_max, pos0, s);
}

// obte_kv_cache_rope_store_rows and obte_kv8_cache_rope_store_rows (a decode step: n = 1): the same checks; who: the entry point named in an error
int rope_store_rows_checked(const char* who, bool e4m3, obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos, int64_t max_pos, int64_t B,
                            int32_t n_head, int32_t head_dim, void* cache, int64_t T_max, obte_stream s) {
    OBTE_REQUIRE(qkv && rope_cos && rope_sin && pos && cache, "%s: null pointer", who);
    OBTE_REQUIRE(shape_ok(B, T_max, n_head, head_dim), "%s: bad shape (head_dim 64 or 128)", who);
    OBTE_REQUIRE(max_pos >= 0 && max_pos < T_max, "%s: max_pos = %lld outside [0, T_max = %lld)", who, (long long)max_pos, (long long)T_max);
    OBTE_REQUIRE((((uintptr_t)qkv | (uintptr_t)cache | (uintptr_t)rope_cos | (uintptr_t)rope_sin) & 15) == 0 && ((uintptr_t)pos & 3) == 0,
                 "%s: qkv, cache and the tables must be 16-byte aligned, pos 4-byte aligned", who);
    return kv_store_launch(who, e4m3, qkv, rope_cos, rope_sin, pos, max_pos, B, 1, n_head, head_dim, cache, T_max, 0, s);
}

// ---- the attention's launch -------------------------------------------------------------------------------------------------------------------
typedef decltype(&attn_decode_kernel<CacheBf16, 64, false, false>) decode_kernel_t;   // (one signature for every instantiation)
template <class Fmt, bool ROWS, bool PARTIAL = false>
decode_kernel_t decode_kernel_for(int head_dim) {
    return head_dim == 128 ? attn_decode_kernel<Fmt, 128, ROWS, PARTIAL> : attn_decode_kernel<Fmt, 64, ROWS, PARTIAL>;
}

// The dispatch on (format, head size, rows) and the two launches: grid (splits, B H) workgroups on the keys, and with more than one split
// the combine.  partial: PARTIAL instead (no combine; the bf16 cache's uniform form only: its one caller, obte_attn_decode_partials).
void launch_decode(bool e4m3, bool partial, int head_dim, const dim3& grid, hipStream_t st, const bf16* q, int64_t q_ld, const void* cache, bf16* o, float* lse,
                   float* ws, int H, int64_t T_max, int n_keys, int per, float qscale, const int32_t* rows_n, int key_off) {
    const decode_kernel_t kernel = partial ? decode_kernel_for<CacheBf16, false, true>(head_dim)
                                   : e4m3  ? (rows_n ? decode_kernel_for<CacheE4m3, true>(head_dim) : decode_kernel_for<CacheE4m3, false>(head_dim))
                                           : (rows_n ? decode_kernel_for<CacheBf16, true>(head_dim) : decode_kernel_for<CacheBf16, false>(head_dim));
    hipLaunchKernelGGL(kernel, grid, dim3(DEC_WAVES * 64), 0, st, q, q_ld, cache, o, lse, ws, H, T_max, (int64_t)grid.y * T_max, n_keys, per, qscale, rows_n, key_off);
    if (partial || grid.x == 1) return;
    if (head_dim == 128) hipLaunchKernelGGL(attn_decode_combine_kernel<128>, dim3(grid.y), dim3(128), 0, st, ws, o, lse, (int)grid.x);
    else hipLaunchKernelGGL(attn_decode_combine_kernel<64>, dim3(grid.y), dim3(64), 0, st, ws, o, lse, (int)grid.x);
}

int keys_per_split(int64_t n_keys, int splits) { return (int)(cdiv64(cdiv64(n_keys, splits), DEC_CHUNK) * DEC_CHUNK); }

}  // namespace

extern "C" int64_t obte_kv_cache_bytes(int64_t B, int64_t T_max, int32_t n_head, int32_t head_dim) {
    return shape_ok(B, T_max, n_head, head_dim) ? 2 * B * n_head * T_max * head_dim * 2 : 0;
}

extern "C" int64_t obte_kv8_cache_bytes(int64_t B, int64_t T_max, int32_t n_head, int32_t head_dim) {
    return shape_ok(B, T_max, n_head, head_dim) ? 2 * B * n_head * T_max * (int64_t)(head_dim + 4) : 0;
}

extern "C" int obte_kv_cache_store(const obte_bf16* qkv, int64_t B, int64_t t, int32_t n_head, int32_t head_dim, obte_bf16* cache, int64_t T_max,
                                   int64_t pos0, obte_stream s) {
    return kv_store_checked("obte_kv_cache_store", false, qkv, B, t, n_head, head_dim, cache, T_max, pos0, s);
}

extern "C" int obte_kv8_cache_store(const obte_bf16* qkv, int64_t B, int64_t t, int32_t n_head, int32_t head_dim, void* cache8, int64_t T_max, int64_t pos0,
                                    obte_stream s) {
    return kv_store_checked("obte_kv8_cache_store", true, qkv, B, t, n_head, head_dim, cache8, T_max, pos0, s);
}

extern "C" int64_t obte_attn_decode_ws_bytes(int64_t B, int32_t n_head, int32_t head_dim) {
    return shape_ok(B, 1, n_head, head_dim) ? B * n_head * OBTE_ATTN_DECODE_MAX_SPLITS * (int64_t)(head_dim + DEC_PAD) * 4 : 0;
}

// The default split count.  A split is worth its workgroup (and the combine launch behind it) only with DEC_MIN_KEYS keys of its own, and
// more than DEC_TARGET_WGS workgroups in all buy nothing: every CU has one (the decode section, has the measurements).
constexpr int64_t DEC_TARGET_WGS = 256;   // 1 per CU
constexpr int64_t DEC_MIN_KEYS = 256;
extern "C" int obte_attn_decode_splits(int64_t B, int32_t n_head, int32_t head_dim, int64_t n_keys) {
    if (!shape_ok(B, 1, n_head, head_dim) || n_keys < 1) return 1;
    const int64_t by_fill = cdiv64(DEC_TARGET_WGS, B * n_head), by_keys = n_keys / DEC_MIN_KEYS;
    int64_t n = by_fill < by_keys ? by_fill : by_keys;
    if (n > OBTE_ATTN_DECODE_MAX_SPLITS) n = OBTE_ATTN_DECODE_MAX_SPLITS;
    return n < 1 ? 1 : (int)n;
}

// The kernel alone with PARTIAL (attention_shared.hip has checked every argument): BH rows of a bf16 cache of T_max positions, every row
// over the keys [0, n_keys), `splits` partials per row to part in this file's layout, the keys divided as obte_attn_decode divides them.
// ancestry (with its group size): the ancestry form, key j of row b read from row b - b % group + ancestry[b * T_max + j].
void obte_attn_decode_partials(int head_dim, int BH, int H, int splits, const bf16* q, int64_t q_ld, const bf16* cache, int64_t T_max, int n_keys, float qscale,
                               float* part, hipStream_t st, const int32_t* ancestry, int group) {
    if (ancestry) {
        const decode_kernel_t kernel = decode_kernel_for<CacheBf16Anc, false, true>(head_dim);
        hipLaunchKernelGGL(kernel, dim3((unsigned)splits, (unsigned)BH), dim3(DEC_WAVES * 64), 0, st, q, q_ld, (const void*)cache, (bf16*)nullptr, (float*)nullptr, part, H,
                           T_max, (int64_t)BH * T_max, n_keys, keys_per_split(n_keys, splits), qscale, ancestry, group);
        return;
    }
    launch_decode(false, true, head_dim, dim3((unsigned)splits, (unsigned)BH), st, q, q_ld, cache, nullptr, nullptr, part, H, T_max, n_keys,
                  keys_per_split(n_keys, splits), qscale, nullptr, 0);
}

// The checks and the launch behind obte_attn_decode, obte_attn_decode_rows and obte_attn_decode_kv8 (and csrc/block.cpp's cached step).
// rows_n null: every row over the keys [0, n_keys).  Else row b over rows_n[b] + key_off keys, n_keys the host's bound on that (the
// kernel forms `per` from the row's own count).
int obte_attn_decode_on(bool e4m3, const char* who, const obte_bf16* q, int64_t q_ld, const void* cache, obte_bf16* o, float* lse, int64_t B, int64_t T_max,
                        int64_t n_keys, const int32_t* rows_n, int32_t key_off, int32_t n_head, int32_t head_dim, float scale, int32_t splits, void* ws,
                        int64_t ws_bytes, obte_stream s) {
    OBTE_REQUIRE(q && cache && o, "%s: null pointer", who);
    OBTE_REQUIRE(shape_ok(B, T_max, n_head, head_dim) && B * n_head <= 65535, "%s: bad shape (head_dim 64 or 128, B * n_head <= 65535)", who);
    OBTE_REQUIRE(n_keys >= 1 && n_keys <= T_max, "%s: %s = %lld outside [1, T_max = %lld]", who, rows_n && !e4m3 ? "max_keys" : "n_keys",   // (each header's name for the bound)
                 (long long)n_keys, (long long)T_max);
    OBTE_REQUIRE(q_ld >= (int64_t)n_head * head_dim && q_ld % 8 == 0, "%s: q_ld must be a multiple of 8 and at least n_head * head_dim", who);
    OBTE_REQUIRE((((uintptr_t)q | (uintptr_t)cache | (uintptr_t)o) & 15) == 0 && ((uintptr_t)rows_n & 3) == 0,
                 "%s: q, cache and o must be 16-byte aligned, a per-row n_keys 4-byte aligned", who);
    OBTE_REQUIRE(splits >= 0 && splits <= OBTE_ATTN_DECODE_MAX_SPLITS, "%s: splits = %d outside [0, %d]", who, splits, OBTE_ATTN_DECODE_MAX_SPLITS);
    if (splits == 0) splits = obte_attn_decode_splits(B, n_head, head_dim, n_keys);
    if (splits > 1) {
        const int64_t need = B * n_head * splits * (int64_t)(head_dim + DEC_PAD) * 4;
        OBTE_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0, "%s: %d splits need a 16-byte aligned workspace of %lld bytes, got %lld", who, splits,
                     (long long)need, (long long)(ws ? ws_bytes : 0));
    }
    const hipStream_t st = (hipStream_t)s;
    const int BH = (int)(B * n_head);
    // cache bytes read = 4 * BH * n_keys * head_dim (e4m3: 2 * BH * n_keys * (head_dim + 4)); rows: the bound, a row reads its own count
    const int prof = obte_prof_begin(st, e4m3 ? 105 : 102, BH, n_keys, head_dim);
    launch_decode(e4m3, false, head_dim, dim3((unsigned)splits, (unsigned)BH), st, (const bf16*)q, q_ld, cache, (bf16*)o, lse, (float*)ws, n_head, T_max, (int)n_keys,
                  rows_n ? 0 : keys_per_split(n_keys, splits), scale * 1.4426950408889634f, rows_n, key_off);
    obte_prof_end(prof, st);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}

extern "C" int obte_attn_decode(const obte_bf16* q, int64_t q_ld, const obte_bf16* cache, obte_bf16* o, float* lse, int64_t B, int64_t T_max, int64_t n_keys,
                                int32_t n_head, int32_t head_dim, float scale, int32_t splits, void* ws, int64_t ws_bytes, obte_stream s) {
    return obte_attn_decode_on(false, "obte_attn_decode", q, q_ld, cache, o, lse, B, T_max, n_keys, nullptr, 0, n_head, head_dim, scale, splits, ws, ws_bytes, s);
}

extern "C" int obte_attn_decode_rows(const obte_bf16* q, int64_t q_ld, const obte_bf16* cache, obte_bf16* o, float* lse, int64_t B, int64_t T_max,
                                     const int32_t* n_keys, int64_t max_keys, int32_t n_head, int32_t head_dim, float scale, int32_t splits, void* ws,
                                     int64_t ws_bytes, obte_stream s) {
    OBTE_REQUIRE(n_keys, "obte_attn_decode_rows: null pointer");   // (here a null count is not the uniform form)
    return obte_attn_decode_on(false, "obte_attn_decode_rows", q, q_ld, cache, o, lse, B, T_max, max_keys, n_keys, 0, n_head, head_dim, scale, splits, ws, ws_bytes, s);
}

extern "C" int obte_attn_decode_kv8(const obte_bf16* q, int64_t q_ld, const void* cache8, obte_bf16* o, float* lse, int64_t B, int64_t T_max, int64_t n_keys,
                                    const int32_t* n_keys_rows, int32_t n_head, int32_t head_dim, float scale, int32_t splits, void* ws, int64_t ws_bytes,
                                    obte_stream s) {
    return obte_attn_decode_on(true, "obte_attn_decode_kv8", q, q_ld, cache8, o, lse, B, T_max, n_keys, n_keys_rows, 0, n_head, head_dim, scale, splits, ws, ws_bytes, s);
}

// ---- one position / key count per row ---------------------------------------------------------------------------------------------------
// The rotate-and-store of n_new positions per row, row b's from pos_rows[b] on (include/omnibiote_hip_extend.h; its shape rule is
// obte_attn_extend's: B * n_head <= 65535, n_new < 2^20, B * n_new < 2^31) ...
extern "C" int obte_kv_cache_rope_store_chunk(obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos_rows, int64_t max_pos, int64_t B,
                                              int64_t n_new, int32_t n_head, int32_t head_dim, obte_bf16* cache, int64_t T_max, obte_stream s) {
    OBTE_REQUIRE(qkv && rope_cos && rope_sin && pos_rows && cache, "obte_kv_cache_rope_store_chunk: null pointer");
    OBTE_REQUIRE(shape_ok(B, T_max, n_head, head_dim) && B * n_head <= 65535 && n_new > 0 && n_new < (1ll << 20) && B * n_new < (1ll << 31),
                 "obte_kv_cache_rope_store_chunk: bad shape (head_dim 64 or 128, n_new >= 1)");
    OBTE_REQUIRE(max_pos >= 0 && max_pos + n_new <= T_max, "obte_kv_cache_rope_store_chunk: positions up to %lld + %lld do not fit T_max = %lld", (long long)max_pos,
                 (long long)n_new, (long long)T_max);
    OBTE_REQUIRE((((uintptr_t)qkv | (uintptr_t)cache | (uintptr_t)rope_cos | (uintptr_t)rope_sin) & 15) == 0 && ((uintptr_t)pos_rows & 3) == 0,
                 "obte_kv_cache_rope_store_chunk: qkv, cache and the tables must be 16-byte aligned, pos_rows 4-byte aligned");
    return kv_store_launch("obte_kv_cache_rope_store_chunk", false, qkv, rope_cos, rope_sin, pos_rows, max_pos, B, n_new, n_head, head_dim, cache, T_max, 0, s);
}

// ... and of one: a decode step (include/omnibiote_hip_rows.h, include/omnibiote_hip_kv8.h).  Their own checks, the same kernel at n = 1.
extern "C" int obte_kv_cache_rope_store_rows(obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos, int64_t max_pos, int64_t B,
                                             int32_t n_head, int32_t head_dim, obte_bf16* cache, int64_t T_max, obte_stream s) {
    return rope_store_rows_checked("obte_kv_cache_rope_store_rows", false, qkv, rope_cos, rope_sin, pos, max_pos, B, n_head, head_dim, cache, T_max, s);
}

extern "C" int obte_kv8_cache_rope_store_rows(obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos, int64_t max_pos, int64_t B,
                                              int32_t n_head, int32_t head_dim, void* cache8, int64_t T_max, obte_stream s) {
    return rope_store_rows_checked("obte_kv8_cache_rope_store_rows", true, qkv, rope_cos, rope_sin, pos, max_pos, B, n_head, head_dim, cache8, T_max, s);
}

// The cached step's store (csrc/block.cpp): n positions per row join the cache, every row's from `pos` on (pos_rows null: the rows are
// rotated already) or row b's from pos_rows[b] on, rotated here (pos: their bound).  Each case is one of the entry points above.
int obte_kv_store_on(bool e4m3, const char* who, obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos_rows, int64_t pos, int64_t B, int64_t n,
                     int32_t n_head, int32_t head_dim, void* cache, int64_t T_max, obte_stream s) {
    if (!pos_rows)
        return e4m3 ? obte_kv8_cache_store(qkv, B, n, n_head, head_dim, cache, T_max, pos, s) : obte_kv_cache_store(qkv, B, n, n_head, head_dim, (obte_bf16*)cache, T_max, pos, s);
    if (e4m3) return rope_store_rows_checked(who, true, qkv, rope_cos, rope_sin, pos_rows, pos, B, n_head, head_dim, cache, T_max, s);   // (n = 1: decode only)
    if (n == 1) return obte_kv_cache_rope_store_rows(qkv, rope_cos, rope_sin, pos_rows, pos, B, n_head, head_dim, (obte_bf16*)cache, T_max, s);
    return obte_kv_cache_rope_store_chunk(qkv, rope_cos, rope_sin, pos_rows, pos, B, n, n_head, head_dim, (obte_bf16*)cache, T_max, s);
}

// ---- the cache in pages (include/omnibiote_hip_paged.h) -------------------------------------------------------------------------------------
namespace {

bool paged_shape_ok(int64_t B, int64_t n_pages, int64_t table_ld, int32_t n_head, int32_t head_dim) {
    return shape_ok(B, 1, n_head, head_dim) && n_pages > 0 && n_pages < (1ll << 24) && table_ld > 0 && table_ld < (1ll << 18);   // (64 table_ld < 2^24, as T_max)
}

// the launch behind the four paged stores, each after its own argument checks: kv_store_launch's, with the table
int kv_paged_store_launch(const char* who, bool e4m3, const obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos_rows, int64_t max_pos,
                          int64_t B, int64_t n, int32_t n_head, int32_t head_dim, void* pool, int64_t n_pages, const int32_t* table, int64_t table_ld, obte_stream s) {
    const int64_t items = B * n * (pos_rows ? 3 : 2) * n_head * head_dim / 8;
    OBTE_REQUIRE(cdiv64(items, 256) < (1ll << 31), "%s: too many rows for one launch", who);
    const auto kernel = pos_rows ? (e4m3 ? kv_store_kernel<CachePaged8, true> : kv_store_kernel<CachePaged, true>)
                                 : (e4m3 ? kv_store_kernel<CachePaged8, false> : kv_store_kernel<CachePaged, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)cdiv64(items, 256)), dim3(256), 0, (hipStream_t)s, (bf16*)qkv, pool, items, table_ld, (int64_t)0,
                       n_pages * n_head * DEC_CHUNK, (int)n, n_head, head_dim, (int)max_pos, rope_cos, rope_sin, pos_rows, table, (int)n_pages);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}

// obte_kv_paged_store and obte_kv8_paged_store: the same checks
int kv_paged_store_checked(const char* who, bool e4m3, const obte_bf16* qkv, int64_t B, int64_t t, int32_t n_head, int32_t head_dim, void* pool, int64_t n_pages,
                           const int32_t* table, int64_t table_ld, obte_stream s) {
    OBTE_REQUIRE(qkv && pool && table, "%s: null pointer", who);
    OBTE_REQUIRE(paged_shape_ok(B, n_pages, table_ld, n_head, head_dim), "%s: bad shape (head_dim 64 or 128)", who);
    OBTE_REQUIRE(t > 0 && t <= DEC_CHUNK * table_ld, "%s: positions [0, %lld) do not fit the table's %lld pages per row", who, (long long)t, (long long)table_ld);
    OBTE_REQUIRE((((uintptr_t)qkv | (uintptr_t)pool) & 15) == 0 && ((uintptr_t)table & 3) == 0, "%s: qkv and pool must be 16-byte aligned, table 4-byte aligned", who);
    return kv_paged_store_launch(who, e4m3, qkv, nullptr, nullptr, nullptr, 0, B, t, n_head, head_dim, pool, n_pages, table, table_ld, s);
}

// obte_kv_paged_rope_store_rows and obte_kv8_paged_rope_store_rows: the same checks
int paged_rope_store_rows_checked(const char* who, bool e4m3, obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos, int64_t max_pos, int64_t B,
                                  int32_t n_head, int32_t head_dim, void* pool, int64_t n_pages, const int32_t* table, int64_t table_ld, obte_stream s) {
    OBTE_REQUIRE(qkv && rope_cos && rope_sin && pos && pool && table, "%s: null pointer", who);
    OBTE_REQUIRE(paged_shape_ok(B, n_pages, table_ld, n_head, head_dim), "%s: bad shape (head_dim 64 or 128)", who);
    OBTE_REQUIRE(max_pos >= 0 && max_pos < DEC_CHUNK * table_ld, "%s: max_pos = %lld outside the table's [0, %lld)", who, (long long)max_pos,
                 (long long)(DEC_CHUNK * table_ld));
    OBTE_REQUIRE((((uintptr_t)qkv | (uintptr_t)pool | (uintptr_t)rope_cos | (uintptr_t)rope_sin) & 15) == 0 && (((uintptr_t)pos | (uintptr_t)table) & 3) == 0,
                 "%s: qkv, pool and the rope tables must be 16-byte aligned, pos and table 4-byte aligned", who);
    return kv_paged_store_launch(who, e4m3, qkv, rope_cos, rope_sin, pos, max_pos, B, 1, n_head, head_dim, pool, n_pages, table, table_ld, s);
}

}  // namespace

extern "C" int64_t obte_kv_paged_bytes(int64_t n_pages, int32_t n_head, int32_t head_dim) {
    return paged_shape_ok(1, n_pages, 1, n_head, head_dim) ? 2 * n_pages * n_head * DEC_CHUNK * head_dim * 2 : 0;
}

extern "C" int64_t obte_kv8_paged_bytes(int64_t n_pages, int32_t n_head, int32_t head_dim) {
    return paged_shape_ok(1, n_pages, 1, n_head, head_dim) ? 2 * n_pages * n_head * DEC_CHUNK * (int64_t)(head_dim + 4) : 0;
}

extern "C" int obte_kv_paged_store(const obte_bf16* qkv, int64_t B, int64_t t, int32_t n_head, int32_t head_dim, obte_bf16* pool, int64_t n_pages,
                                   const int32_t* table, int64_t table_ld, obte_stream s) {
    return kv_paged_store_checked("obte_kv_paged_store", false, qkv, B, t, n_head, head_dim, pool, n_pages, table, table_ld, s);
}

extern "C" int obte_kv8_paged_store(const obte_bf16* qkv, int64_t B, int64_t t, int32_t n_head, int32_t head_dim, void* pool8, int64_t n_pages, const int32_t* table,
                                    int64_t table_ld, obte_stream s) {
    return kv_paged_store_checked("obte_kv8_paged_store", true, qkv, B, t, n_head, head_dim, pool8, n_pages, table, table_ld, s);
}

extern "C" int obte_kv_paged_rope_store_rows(obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos, int64_t max_pos, int64_t B,
                                             int32_t n_head, int32_t head_dim, obte_bf16* pool, int64_t n_pages, const int32_t* table, int64_t table_ld,
                                             obte_stream s) {
    return paged_rope_store_rows_checked("obte_kv_paged_rope_store_rows", false, qkv, rope_cos, rope_sin, pos, max_pos, B, n_head, head_dim, pool, n_pages, table,
                                         table_ld, s);
}

extern "C" int obte_kv8_paged_rope_store_rows(obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos, int64_t max_pos, int64_t B,
                                              int32_t n_head, int32_t head_dim, void* pool8, int64_t n_pages, const int32_t* table, int64_t table_ld,
                                              obte_stream s) {
    return paged_rope_store_rows_checked("obte_kv8_paged_rope_store_rows", true, qkv, rope_cos, rope_sin, pos, max_pos, B, n_head, head_dim, pool8, n_pages, table,
                                         table_ld, s);
}

// n_new positions per row from pos_rows[b] on, through the table (include/omnibiote_hip_paged_extend.h): obte_kv_cache_rope_store_chunk's shape rule and
// bound with 64 table_ld in T_max's place, the paged stores' launch at n = n_new
extern "C" int obte_kv_paged_rope_store_chunk(obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos_rows, int64_t max_pos, int64_t B,
                                              int64_t n_new, int32_t n_head, int32_t head_dim, obte_bf16* pool, int64_t n_pages, const int32_t* table, int64_t table_ld,
                                              obte_stream s) {
    const char* who = "obte_kv_paged_rope_store_chunk";
    OBTE_REQUIRE(qkv && rope_cos && rope_sin && pos_rows && pool && table, "%s: null pointer", who);
    OBTE_REQUIRE(paged_shape_ok(B, n_pages, table_ld, n_head, head_dim) && B * n_head <= 65535 && n_new > 0 && n_new < (1ll << 20) && B * n_new < (1ll << 31),
                 "%s: bad shape (head_dim 64 or 128, n_new >= 1)", who);
    OBTE_REQUIRE(max_pos >= 0 && max_pos + n_new <= DEC_CHUNK * table_ld, "%s: positions up to %lld + %lld do not fit the table's [0, 64 * table_ld = %lld)", who,
                 (long long)max_pos, (long long)n_new, (long long)(DEC_CHUNK * table_ld));
    OBTE_REQUIRE((((uintptr_t)qkv | (uintptr_t)pool | (uintptr_t)rope_cos | (uintptr_t)rope_sin) & 15) == 0 && (((uintptr_t)pos_rows | (uintptr_t)table) & 3) == 0,
                 "%s: qkv, pool and the rope tables must be 16-byte aligned, pos_rows and table 4-byte aligned", who);
    return kv_paged_store_launch(who, false, qkv, rope_cos, rope_sin, pos_rows, max_pos, B, n_new, n_head, head_dim, pool, n_pages, table, table_ld, s);
}

// obte_attn_decode_on's checks and its two launches, on the pool (e4m3: the pool of include/omnibiote_hip_paged8.h): row b over rows_n[b] + key_off keys,
// max_keys the host's bound on that
int obte_attn_decode_paged_on(bool e4m3, const char* who, const obte_bf16* q, int64_t q_ld, const void* pool, int64_t n_pages, const int32_t* table, int64_t table_ld,
                              obte_bf16* o, float* lse, int64_t B, const int32_t* rows_n, int32_t key_off, int64_t max_keys, int32_t n_head, int32_t head_dim,
                              float scale, int32_t splits, void* ws, int64_t ws_bytes, obte_stream s) {
    OBTE_REQUIRE(q && pool && table && o && rows_n, "%s: null pointer", who);
    OBTE_REQUIRE(paged_shape_ok(B, n_pages, table_ld, n_head, head_dim) && B * n_head <= 65535, "%s: bad shape (head_dim 64 or 128, B * n_head <= 65535)", who);
    OBTE_REQUIRE(max_keys >= 1 && max_keys <= DEC_CHUNK * table_ld, "%s: max_keys = %lld outside [1, 64 * table_ld = %lld]", who, (long long)max_keys,
                 (long long)(DEC_CHUNK * table_ld));
    OBTE_REQUIRE(q_ld >= (int64_t)n_head * head_dim && q_ld % 8 == 0, "%s: q_ld must be a multiple of 8 and at least n_head * head_dim", who);
    OBTE_REQUIRE((((uintptr_t)q | (uintptr_t)pool | (uintptr_t)o) & 15) == 0 && (((uintptr_t)rows_n | (uintptr_t)table) & 3) == 0,
                 "%s: q, pool and o must be 16-byte aligned, n_keys and table 4-byte aligned", who);
    OBTE_REQUIRE(splits >= 0 && splits <= OBTE_ATTN_DECODE_MAX_SPLITS, "%s: splits = %d outside [0, %d]", who, splits, OBTE_ATTN_DECODE_MAX_SPLITS);
    if (splits == 0) splits = obte_attn_decode_splits(B, n_head, head_dim, max_keys);
    if (splits > 1) {
        const int64_t need = B * n_head * splits * (int64_t)(head_dim + DEC_PAD) * 4;
        OBTE_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0, "%s: %d splits need a 16-byte aligned workspace of %lld bytes, got %lld", who, splits,
                     (long long)need, (long long)(ws ? ws_bytes : 0));
    }
    const hipStream_t st = (hipStream_t)s;
    const int BH = (int)(B * n_head);
    const int prof = obte_prof_begin(st, e4m3 ? 119 : 102, BH, max_keys, head_dim);
    const auto kernel = e4m3 ? (head_dim == 128 ? attn_decode_paged_kernel<CachePaged8, 128> : attn_decode_paged_kernel<CachePaged8, 64>)
                             : (head_dim == 128 ? attn_decode_paged_kernel<CachePaged, 128> : attn_decode_paged_kernel<CachePaged, 64>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)splits, (unsigned)BH), dim3(DEC_WAVES * 64), 0, st, (const bf16*)q, q_ld, pool, (bf16*)o, lse, (float*)ws,
                       n_head, table_ld, (int)n_pages, (int)max_keys, scale * 1.4426950408889634f, rows_n, key_off, table);
    if (splits > 1) {
        if (head_dim == 128) hipLaunchKernelGGL(attn_decode_combine_kernel<128>, dim3((unsigned)BH), dim3(128), 0, st, (const float*)ws, (bf16*)o, lse, (int)splits);
        else hipLaunchKernelGGL(attn_decode_combine_kernel<64>, dim3((unsigned)BH), dim3(64), 0, st, (const float*)ws, (bf16*)o, lse, (int)splits);
    }
    obte_prof_end(prof, st);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}

extern "C" int obte_attn_decode_paged(const obte_bf16* q, int64_t q_ld, const obte_bf16* pool, int64_t n_pages, const int32_t* table, int64_t table_ld,
                                      obte_bf16* o, float* lse, int64_t B, const int32_t* n_keys, int64_t max_keys, int32_t n_head, int32_t head_dim, float scale,
                                      int32_t splits, void* ws, int64_t ws_bytes, obte_stream s) {
    return obte_attn_decode_paged_on(false, "obte_attn_decode_paged", q, q_ld, pool, n_pages, table, table_ld, o, lse, B, n_keys, 0, max_keys, n_head, head_dim, scale,
                                     splits, ws, ws_bytes, s);
}

extern "C" int obte_attn_decode_paged8(const obte_bf16* q, int64_t q_ld, const void* pool8, int64_t n_pages, const int32_t* table, int64_t table_ld, obte_bf16* o,
                                       float* lse, int64_t B, const int32_t* n_keys, int64_t max_keys, int32_t n_head, int32_t head_dim, float scale, int32_t splits,
                                       void* ws, int64_t ws_bytes, obte_stream s) {
    return obte_attn_decode_paged_on(true, "obte_attn_decode_paged8", q, q_ld, pool8, n_pages, table, table_ld, o, lse, B, n_keys, 0, max_keys, n_head, head_dim, scale,
                                     splits, ws, ws_bytes, s);
}
