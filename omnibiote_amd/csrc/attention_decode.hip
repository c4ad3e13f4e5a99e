// Autoregressive generation: the key/value cache and attention for ONE query per (batch, head) (include/omnibiote_hip.h,
// "autoregressive generation"; extends training/model.py:115-130, whose generate() the reference struck out).
//
// The cache of one layer is K [B, H, T_max, hs] followed by V in the same shape, bf16: a (b, h)'s keys are hs * 2 bytes apart, so a
// step streams them as one contiguous run.  obte_kv_cache_store copies the k and v thirds of a packed qkv activation there.
//
// obte_attn_decode is bound by the read of the cache: 4 hs bytes per key against 4 hs flops.  No MFMA, no LDS staging:
//   - grid (split, b H + h); a workgroup of 4 waves owns the keys [k0, k1) of its split.  hs / 8 lanes share one key, each holding 16
//     bytes (8 dims) of its K row and of its V row: a wave's load instruction covers 1 KiB of consecutive rows, and the lane that
//     multiplies dims 8c .. 8c+7 of q by K is the one that accumulates those dims of P V.  UNROLL keys per lane group are loaded (K and
//     V: 2 UNROLL 16-byte loads in flight per lane) before the first of them is used.
//   - q sits in 8 fp32 registers per lane with scale * log2(e) folded in; a score is 8 FMAs and a DPP sum over the key's lanes.  Every
//     lane group runs its own online softmax (m, l, acc[8] in fp32, exp2 domain): nothing crosses lanes inside the loop but the score.
//   - the groups of a wave merge by lane exchange, the waves through LDS in wave order; the workgroup writes o / lse itself (one split)
//     or an fp32 partial (acc[hs], m, l) to the workspace, which a second launch combines in split order.  No atomics, no flags.
//   - a key at or beyond k1 never enters: its loads are redirected to the split's last key, its score is -inf, its weight an exact 0
//     and its V a selected 0, so whatever the cache holds past n_keys (NaN patterns included) cannot reach the result.  A lane group,
//     a wave or a split without any key carries (m = -inf, l = 0, acc = 0); every merge rescales against a maximum made finite first,
//     so exp2(-inf - -inf) is never formed.
//
// The rows forms (obte_kv_cache_rope_store_rows and its n-positions form obte_kv_cache_rope_store_chunk, one kernel; obte_attn_decode_rows):
// one position / key count PER ROW, an int32 the kernels read on the device, for a batch whose rows stand at different positions.  A value outside the host's bound makes the row inactive: nothing
// of it is stored, none of its cache is read, its attention output is exact zeros and its lse -inf — an out-of-range device value is
// memory-safe without a status word, and a negative one parks a finished row.  The attention kernel is the one above with ROWS = true:
// a workgroup derives its key range from its own row's count by the host's formula, so a row of n keys under s splits is partitioned
// (and summed) exactly as obte_attn_decode partitions n keys under s splits.
#include "common.h"

namespace {

// (DEC_WAVES, DEC_UNROLL, DEC_CHUNK, DEC_PAD: common.h — attention_kv8.hip shares the partition and the partial layout)

__device__ __forceinline__ void unpack8(u32x4 r, float* f) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[2 * j] = __builtin_bit_cast(float, r[j] << 16);
        f[2 * j + 1] = __builtin_bit_cast(float, r[j] & 0xFFFF0000u);
    }
}

// sum over the LPR (8 or 16) consecutive lanes that share a key: every one of them gets the total
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
    v += dpp_moved<0xB1>(v);          // quad_perm [1,0,3,2]
    v += dpp_moved<0x4E>(v);          // quad_perm [2,3,0,1]
    v += dpp_moved<0x141>(v);         // row_half_mirror: 8 lanes
    if (LPR == 16) v += dpp_moved<0x140>(v);   // row_mirror: 16 lanes
    return v;
}

struct Part { float m, l, acc[8]; };   // one online-softmax state, exp2 domain: sum_k exp2(s_k - m) (1, v_k) for the 8 dims of a lane

// a += b with both rescaled to the common maximum; an empty side (m = -inf, l = 0, acc = 0) adds exactly nothing
__device__ __forceinline__ void merge(Part& a, const Part& b) {
    const float m = fmaxf(a.m, b.m);
    const float ms = m == -INFINITY ? 0.f : m;
    const float wa = __builtin_amdgcn_exp2f(a.m - ms), wb = __builtin_amdgcn_exp2f(b.m - ms);
    a.m = m;
    a.l = a.l * wa + b.l * wb;
#pragma unroll
    for (int j = 0; j < 8; ++j) a.acc[j] = a.acc[j] * wa + b.acc[j] * wb;
}

// UNROLL keys of one lane group.  TAIL: some of them may lie at or beyond k1.
template <int LPR, bool TAIL>
__device__ __forceinline__ void decode_keys(Part& st, const float* qf, const bf16* kb, const bf16* vb, int hs, int key0, int kstride, int k1, int chunk) {
    u32x4 kr[DEC_UNROLL], vr[DEC_UNROLL];
    bool ok[DEC_UNROLL];
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
        const int key = key0 + u * kstride;
        ok[u] = !TAIL || key < k1;
        const int64_t off = (int64_t)(ok[u] ? key : k1 - 1) * hs + chunk * 8;   // (k1 - 1 >= k0: a workgroup with no key never gets here)
        kr[u] = *(const u32x4*)(kb + off);
        vr[u] = *(const u32x4*)(vb + off);
    }
    float sc[DEC_UNROLL];
    float mx = st.m;
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
        float kf[8];
        unpack8(kr[u], kf);
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d = __builtin_fmaf(qf[j], kf[j], d);
        d = group_sum<LPR>(d);
        sc[u] = ok[u] ? d : -INFINITY;
        mx = fmaxf(mx, sc[u]);
    }
    const float ms = (TAIL && mx == -INFINITY) ? 0.f : mx;
    const float alpha = __builtin_amdgcn_exp2f(st.m - ms);
    st.m = mx;
    st.l *= alpha;
#pragma unroll
    for (int j = 0; j < 8; ++j) st.acc[j] *= alpha;
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
        const float p = ok[u] ? __builtin_amdgcn_exp2f(sc[u] - ms) : 0.f;
        float vf[8];
        unpack8(ok[u] ? vr[u] : u32x4{0u, 0u, 0u, 0u}, vf);
        st.l += p;
#pragma unroll
        for (int j = 0; j < 8; ++j) st.acc[j] = __builtin_fmaf(p, vf[j], st.acc[j]);
    }
}

// HS: 64 or 128.  grid (splits, B * H), DEC_WAVES * 64 threads.  per: keys per split (a multiple of DEC_CHUNK).
// splits == 1: o and lse are final.  Else part[(bh * splits + split) * (HS + DEC_PAD)] = (acc[HS], m, l).
// ROWS: row b has rows_n[b] + rows_off keys if that lies in [1, n_keys] (n_keys: the host's bound), else none (an inactive row: no
// key is loaded, the state stays (m = -inf, l = 0, acc = 0)); per is formed here from the row's own count.
// PARTIAL (the suffix part of obte_attn_decode_shared, attention_shared.hip): the state leaves as a partial at one split too, o and lse
// are not touched.
template <int HS, bool ROWS, bool PARTIAL = false>
__global__ __launch_bounds__(DEC_WAVES * 64) void attn_decode_kernel(const bf16* __restrict__ q, int64_t q_ld, const bf16* __restrict__ cache,
                                                                      bf16* __restrict__ o, float* __restrict__ lse, float* __restrict__ part,
                                                                      int H, int64_t T_max, int64_t v_off, int n_keys, int per, float qscale,
                                                                      const int32_t* __restrict__ rows_n, int rows_off) {
    constexpr int LPR = HS / 8;        // lanes per key
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

    float qf[8];
    unpack8(*(const u32x4*)(q + b * q_ld + h * HS + chunk * 8), qf);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[j] *= qscale;

    const bf16* kb = cache + (int64_t)bh * T_max * HS;
    const bf16* vb = kb + v_off;
    Part st;
    st.m = -INFINITY; st.l = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) st.acc[j] = 0.f;

    constexpr int KSTRIDE = DEC_WAVES * G;              // keys between two of a lane group's UNROLL keys
    constexpr int ROUND = KSTRIDE * DEC_UNROLL;         // keys of one workgroup round
    const int full_end = k0 + (k1 - k0) / ROUND * ROUND;
    int base = k0;
    for (; base < full_end; base += ROUND) decode_keys<LPR, false>(st, qf, kb, vb, HS, base + wave * G + grp, KSTRIDE, k1, chunk);
    if (base < k1) decode_keys<LPR, true>(st, qf, kb, vb, HS, base + wave * G + grp, KSTRIDE, k1, chunk);   // (workgroup-uniform)

    // the lane groups of a wave: exchange with the lane LPR, 2 LPR, .. 32 away (the same dims of another key's state)
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1) {
        Part other;
        other.m = __shfl_xor(st.m, off, 64); other.l = __shfl_xor(st.l, off, 64);
#pragma unroll
        for (int j = 0; j < 8; ++j) other.acc[j] = __shfl_xor(st.acc[j], off, 64);
        // both partners must add in one order for the result to be the same on each: the lower lane's state first
        if (lane & off) { Part t = other; merge(t, st); st = t; }
        else merge(st, other);
    }
    // the waves, through LDS, in wave order
    __shared__ float lds[DEC_WAVES][LPR][10];
    if (lane < LPR) {
        lds[wave][lane][0] = st.m; lds[wave][lane][1] = st.l;
#pragma unroll
        for (int j = 0; j < 8; ++j) lds[wave][lane][2 + j] = st.acc[j];
    }
    __syncthreads();
    if (threadIdx.x >= LPR) return;
    Part tot;
    tot.m = lds[0][lane][0]; tot.l = lds[0][lane][1];
#pragma unroll
    for (int j = 0; j < 8; ++j) tot.acc[j] = lds[0][lane][2 + j];
#pragma unroll
    for (int w = 1; w < DEC_WAVES; ++w) {
        Part p;
        p.m = lds[w][lane][0]; p.l = lds[w][lane][1];
#pragma unroll
        for (int j = 0; j < 8; ++j) p.acc[j] = lds[w][lane][2 + j];
        merge(tot, p);
    }
    if (!PARTIAL && splits == 1) {   // n_keys >= 1: l > 0; an inactive row (ROWS): l = 0, o = 0 and lse = -inf
        const float inv = (ROWS && tot.l == 0.f) ? 0.f : 1.0f / tot.l;
        bf16x8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j) out[j] = f2bf(tot.acc[j] * inv);
        *(bf16x8*)(o + ((int64_t)bh * HS + lane * 8)) = out;
        if (lse && lane == 0)
            lse[bh] = (ROWS && tot.l == 0.f) ? -INFINITY : (tot.m + __builtin_amdgcn_logf(tot.l)) * 0.6931471805599453f;   // v_log_f32 is log2
        return;
    }
    float* pr = part + ((int64_t)bh * splits + split) * (HS + DEC_PAD);
    *(f32x4*)(pr + lane * 8) = f32x4{tot.acc[0], tot.acc[1], tot.acc[2], tot.acc[3]};
    *(f32x4*)(pr + lane * 8 + 4) = f32x4{tot.acc[4], tot.acc[5], tot.acc[6], tot.acc[7]};
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

// one thread per 16 bytes: item = ((row * 2 + which) * C + column) / 8 of the k (which = 0) and v thirds of qkv
__global__ __launch_bounds__(256) void kv_cache_store_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ cache, int64_t items, int t, int H, int hs,
                                                             int64_t T_max, int64_t pos0, int64_t v_off) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int C = H * hs, cpr = C / 8;             // 16-byte items per third of a row
    const int c8 = (int)(i % cpr);
    const int64_t rw = i / cpr;
    const int which = (int)(rw & 1);
    const int64_t row = rw >> 1;                   // b * t + ti
    const int64_t b = row / t, ti = row % t;
    const int col = c8 * 8, h = col / hs, e = col % hs;
    const u32x4 v = *(const u32x4*)(qkv + row * 3 * C + (1 + which) * C + col);
    *(u32x4*)(cache + which * v_off + ((b * H + h) * T_max + pos0 + ti) * hs + e) = v;
}

// The rows form's rotate-and-store of a chunk, one thread per 16 bytes of the packed qkv [B n, 3C]: item = (row * 3 + third) * C / 8 + c8,
// row = b n + j at position p = pos[b] + j (0 <= pos[b] <= max_pos; any other value: the row is left alone).  The q and k thirds are rotated
// in place by row p of the tables, in the arithmetic of the GEMM epilogue OBTE_EPI_ROPE_QK (fp32 on the bf16 values, the same expression:
// the same bits); the rotated k and the v go to cache position p of the item's head.  n = 1 is one decode step (obte_kv_cache_rope_store_rows).
// Both entry points bound B n below 2^31: a row index divides in 32 bits.
__global__ __launch_bounds__(256) void kv_cache_rope_store_chunk_kernel(bf16* __restrict__ qkv, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                                        const int32_t* __restrict__ pos, int max_pos, int n, bf16* __restrict__ cache, int64_t items,
                                                                        int H, int hs, int64_t T_max, int64_t v_off) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int C = H * hs, cpr = C / 8;
    const int c8 = (int)(i % cpr);
    const int64_t rw = i / cpr;
    const int third = (int)(rw % 3);
    const int row = (int)(rw / 3), b = row / n;
    const int p0 = pos[b];
    if (p0 < 0 || p0 > max_pos) return;
    const int64_t p = (int64_t)p0 + (row - b * n);
    const int col = c8 * 8, h = col / hs, e = col % hs;
    bf16* ptr = qkv + (int64_t)row * 3 * C + third * C + col;
    bf16x8 v = *reinterpret_cast<const bf16x8*>(ptr);
    if (third < 2) {
        const f32x4 c = *reinterpret_cast<const f32x4*>(cos_t + p * (hs / 2) + e / 2);
        const f32x4 sn = *reinterpret_cast<const f32x4*>(sin_t + p * (hs / 2) + e / 2);
        bf16x8 rt;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xe = bf2f(v[2 * j]), xo = bf2f(v[2 * j + 1]);
            rt[2 * j] = f2bf(xe * c[j] - xo * sn[j]);
            rt[2 * j + 1] = f2bf(xe * sn[j] + xo * c[j]);
        }
        v = rt;
        *reinterpret_cast<bf16x8*>(ptr) = v;
    }
    if (third > 0) *reinterpret_cast<bf16x8*>(cache + (third - 1) * v_off + (((int64_t)b * H + h) * T_max + p) * hs + e) = v;
}

bool shape_ok(int64_t B, int64_t T_max, int32_t n_head, int32_t head_dim) {
    return B > 0 && B < (1ll << 31) && T_max > 0 && T_max < (1ll << 24) && n_head > 0 && n_head <= 1024 && (head_dim == 64 || head_dim == 128) &&
           B * n_head < (1ll << 31);
}

// the launch behind obte_kv_cache_rope_store_chunk and obte_kv_cache_rope_store_rows (n_new = 1), each after its own argument checks
int rope_store_launch(const char* who, obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos_rows, int64_t max_pos, int64_t B,
                      int64_t n_new, int32_t n_head, int32_t head_dim, obte_bf16* cache, int64_t T_max, obte_stream s) {
    const int64_t items = B * n_new * 3 * n_head * head_dim / 8;
    OBTE_REQUIRE(cdiv64(items, 256) < (1ll << 31), "%s: too many rows for one launch", who);
    hipLaunchKernelGGL(kv_cache_rope_store_chunk_kernel, dim3((unsigned)cdiv64(items, 256)), dim3(256), 0, (hipStream_t)s, (bf16*)qkv, rope_cos, rope_sin, pos_rows,
                       (int)max_pos, (int)n_new, (bf16*)cache, items, n_head, head_dim, T_max, B * n_head * T_max * head_dim);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}

}  // namespace

extern "C" int64_t obte_kv_cache_bytes(int64_t B, int64_t T_max, int32_t n_head, int32_t head_dim) {
    return shape_ok(B, T_max, n_head, head_dim) ? 2 * B * n_head * T_max * head_dim * 2 : 0;
}

extern "C" int obte_kv_cache_store(const obte_bf16* qkv, int64_t B, int64_t t, int32_t n_head, int32_t head_dim, obte_bf16* cache, int64_t T_max,
                                   int64_t pos0, obte_stream s) {
    OBTE_REQUIRE(qkv && cache, "obte_kv_cache_store: null pointer");
    OBTE_REQUIRE(shape_ok(B, T_max, n_head, head_dim), "obte_kv_cache_store: bad shape (head_dim 64 or 128)");
    OBTE_REQUIRE(t > 0 && pos0 >= 0 && pos0 + t <= T_max, "obte_kv_cache_store: positions [%lld, %lld) do not fit T_max = %lld", (long long)pos0,
                 (long long)(pos0 + t), (long long)T_max);
    OBTE_REQUIRE((((uintptr_t)qkv | (uintptr_t)cache) & 15) == 0, "obte_kv_cache_store: qkv and cache must be 16-byte aligned");
    const int64_t items = B * t * 2 * n_head * head_dim / 8;
    OBTE_REQUIRE(cdiv64(items, 256) < (1ll << 31), "obte_kv_cache_store: too many rows for one launch");
    hipLaunchKernelGGL(kv_cache_store_kernel, dim3((unsigned)cdiv64(items, 256)), dim3(256), 0, (hipStream_t)s, (const bf16*)qkv, (bf16*)cache, items, (int)t,
                       n_head, head_dim, T_max, pos0, B * n_head * T_max * head_dim);
    OBTE_CHECK_LAUNCH("obte_kv_cache_store");
    return OBTE_OK;
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

// the combine launch behind a split launch of this file's kernel or of attention_kv8.hip's (the same partials)
void obte_attn_decode_combine(int head_dim, int BH, int splits, const float* ws, bf16* o, float* lse, hipStream_t st) {
    if (head_dim == 128) hipLaunchKernelGGL(attn_decode_combine_kernel<128>, dim3(BH), dim3(128), 0, st, ws, o, lse, splits);
    else hipLaunchKernelGGL(attn_decode_combine_kernel<64>, dim3(BH), dim3(64), 0, st, ws, o, lse, splits);
}

// The kernel alone with PARTIAL (attention_shared.hip has checked every argument): BH rows of a cache of T_max positions, every row over
// the keys [0, n_keys), `splits` partials per row to part in this file's layout, the keys divided as obte_attn_decode divides them.
void obte_attn_decode_partials(int head_dim, int BH, int H, int splits, const bf16* q, int64_t q_ld, const bf16* cache, int64_t T_max, int n_keys, float qscale,
                               float* part, hipStream_t st) {
    const int per = (int)(cdiv64(cdiv64(n_keys, splits), DEC_CHUNK) * DEC_CHUNK);
    const dim3 grid((unsigned)splits, (unsigned)BH);
    const int64_t v_off = (int64_t)BH * T_max * head_dim;
    if (head_dim == 128)
        hipLaunchKernelGGL((attn_decode_kernel<128, false, true>), grid, dim3(DEC_WAVES * 64), 0, st, q, q_ld, cache, nullptr, nullptr, part, H, T_max, v_off, n_keys, per, qscale, nullptr, 0);
    else
        hipLaunchKernelGGL((attn_decode_kernel<64, false, true>), grid, dim3(DEC_WAVES * 64), 0, st, q, q_ld, cache, nullptr, nullptr, part, H, T_max, v_off, n_keys, per, qscale, nullptr, 0);
}

// obte_attn_decode (rows_n null: every row over the keys [0, n_keys)) and obte_attn_decode_rows_off (ROWS: row b over rows_n[b] + key_off keys,
// n_keys the host's bound on that, the kernel forming `per` from the row's own count): the same checks, the same launch
template <int HS, bool ROWS>
static void launch_decode(const dim3& grid, hipStream_t st, const bf16* q, int64_t q_ld, const bf16* cache, bf16* o, float* lse, float* ws, int H, int64_t T_max,
                          int64_t v_off, int n_keys, int per, float qscale, const int32_t* rows_n, int key_off) {
    hipLaunchKernelGGL((attn_decode_kernel<HS, ROWS>), grid, dim3(DEC_WAVES * 64), 0, st, q, q_ld, cache, o, lse, ws, H, T_max, v_off, n_keys, per, qscale, rows_n, key_off);
    if (grid.x > 1) obte_attn_decode_combine(HS, (int)grid.y, (int)grid.x, ws, o, lse, st);
}

template <bool ROWS>
static int attn_decode_checked(const char* who, const obte_bf16* q, int64_t q_ld, const obte_bf16* cache, obte_bf16* o, float* lse, int64_t B, int64_t T_max,
                               int64_t n_keys, const int32_t* rows_n, int32_t key_off, int32_t n_head, int32_t head_dim, float scale, int32_t splits, void* ws,
                               int64_t ws_bytes, obte_stream s) {
    OBTE_REQUIRE(q && cache && o && (!ROWS || rows_n), "%s: null pointer", who);
    OBTE_REQUIRE(shape_ok(B, T_max, n_head, head_dim) && B * n_head <= 65535, "%s: bad shape (head_dim 64 or 128, B * n_head <= 65535)", who);
    OBTE_REQUIRE(n_keys >= 1 && n_keys <= T_max, "%s: %s = %lld outside [1, T_max = %lld]", who, ROWS ? "max_keys" : "n_keys", (long long)n_keys, (long long)T_max);
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
    const int per = ROWS ? 0 : (int)(cdiv64(cdiv64(n_keys, splits), DEC_CHUNK) * DEC_CHUNK);
    const hipStream_t st = (hipStream_t)s;
    const int BH = (int)(B * n_head);
    const float qscale = scale * 1.4426950408889634f;
    const int64_t v_off = B * n_head * T_max * head_dim;
    const int prof = obte_prof_begin(st, 102, BH, n_keys, head_dim);   // cache bytes read = 4 * BH * n_keys * head_dim (ROWS: the bound, a row reads its own count)
    const dim3 grid((unsigned)splits, (unsigned)BH);
    if (head_dim == 128)
        launch_decode<128, ROWS>(grid, st, (const bf16*)q, q_ld, (const bf16*)cache, (bf16*)o, lse, (float*)ws, n_head, T_max, v_off, (int)n_keys, per, qscale, rows_n, key_off);
    else
        launch_decode<64, ROWS>(grid, st, (const bf16*)q, q_ld, (const bf16*)cache, (bf16*)o, lse, (float*)ws, n_head, T_max, v_off, (int)n_keys, per, qscale, rows_n, key_off);
    obte_prof_end(prof, st);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}

extern "C" int obte_attn_decode(const obte_bf16* q, int64_t q_ld, const obte_bf16* cache, obte_bf16* o, float* lse, int64_t B, int64_t T_max, int64_t n_keys,
                                int32_t n_head, int32_t head_dim, float scale, int32_t splits, void* ws, int64_t ws_bytes, obte_stream s) {
    return attn_decode_checked<false>("obte_attn_decode", q, q_ld, cache, o, lse, B, T_max, n_keys, nullptr, 0, n_head, head_dim, scale, splits, ws, ws_bytes, s);
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
    return rope_store_launch("obte_kv_cache_rope_store_chunk", qkv, rope_cos, rope_sin, pos_rows, max_pos, B, n_new, n_head, head_dim, cache, T_max, s);
}

// ... and of one: a decode step (include/omnibiote_hip_rows.h).  Its own checks, the same kernel at n = 1.
extern "C" int obte_kv_cache_rope_store_rows(obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos, int64_t max_pos, int64_t B,
                                             int32_t n_head, int32_t head_dim, obte_bf16* cache, int64_t T_max, obte_stream s) {
    OBTE_REQUIRE(qkv && rope_cos && rope_sin && pos && cache, "obte_kv_cache_rope_store_rows: null pointer");
    OBTE_REQUIRE(shape_ok(B, T_max, n_head, head_dim), "obte_kv_cache_rope_store_rows: bad shape (head_dim 64 or 128)");
    OBTE_REQUIRE(max_pos >= 0 && max_pos < T_max, "obte_kv_cache_rope_store_rows: max_pos = %lld outside [0, T_max = %lld)", (long long)max_pos, (long long)T_max);
    OBTE_REQUIRE((((uintptr_t)qkv | (uintptr_t)cache | (uintptr_t)rope_cos | (uintptr_t)rope_sin) & 15) == 0 && ((uintptr_t)pos & 3) == 0,
                 "obte_kv_cache_rope_store_rows: qkv, cache and the tables must be 16-byte aligned, pos 4-byte aligned");
    return rope_store_launch("obte_kv_cache_rope_store_rows", qkv, rope_cos, rope_sin, pos, max_pos, B, 1, n_head, head_dim, cache, T_max, s);
}

// obte_attn_decode_rows with row b's count read as n_keys[b] + key_off (csrc/block.cpp hands the positions and 1: no launch to form pos + 1)
int obte_attn_decode_rows_off(const char* who, const obte_bf16* q, int64_t q_ld, const obte_bf16* cache, obte_bf16* o, float* lse, int64_t B, int64_t T_max,
                              const int32_t* n_keys, int32_t key_off, int64_t max_keys, int32_t n_head, int32_t head_dim, float scale, int32_t splits, void* ws,
                              int64_t ws_bytes, obte_stream s) {
    return attn_decode_checked<true>(who, q, q_ld, cache, o, lse, B, T_max, max_keys, n_keys, key_off, n_head, head_dim, scale, splits, ws, ws_bytes, s);
}

extern "C" int obte_attn_decode_rows(const obte_bf16* q, int64_t q_ld, const obte_bf16* cache, obte_bf16* o, float* lse, int64_t B, int64_t T_max,
                                     const int32_t* n_keys, int64_t max_keys, int32_t n_head, int32_t head_dim, float scale, int32_t splits, void* ws,
                                     int64_t ws_bytes, obte_stream s) {
    return obte_attn_decode_rows_off("obte_attn_decode_rows", q, q_ld, cache, o, lse, B, T_max, n_keys, 0, max_keys, n_head, head_dim, scale, splits, ws, ws_bytes, s);
}
