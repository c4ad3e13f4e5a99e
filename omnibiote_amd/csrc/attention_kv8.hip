// The key/value cache in OCP e4m3 (include/omnibiote_hip_kv8.h; the format in words and in plain torch: omnibiote_amd/kvquant.py).
//
// One layer's cache: K codes uint8 [B, H, T_max, hs], V codes in the same shape, K scales fp32 [B, H, T_max], V scales: 2 (hs + 4)
// bytes per (b, h, position) against the bf16 cache's 4 hs.  A head vector x of hs bf16 values is stored as code_i = RNE_e4m3(x_i 2^-e)
// and scale = 2^e, e the smallest integer >= -126 with max|x_i| 2^-e <= 448: a power of two, so the product is exact, the only rounding
// is the conversion's, nothing saturates, and the cache is a pure function of the bf16 inputs.
//
// The store kernel (kv8_store_kernel): hs / 8 lanes share a head vector, 16 bytes of the bf16 input each; the maximum over them by DPP,
// the exponent from the maximum's bits in integer arithmetic, 8 codes per lane from v_cvt_pk_fp8_f32 in one 8-byte store, the scale from
// the vector's first lane.  ROPE: the rows form's rotate-and-store (kv_cache_rope_store_chunk_kernel at n = 1, the same expression, the
// same bits left in qkv), the rotated k and the v quantised.
//
// attn_decode_kv8_kernel is attn_decode_kernel (csrc/attention_decode.hip) on this cache: grid (split, b H + h), 4 waves, a lane group
// per key, global -> VGPR loads, DEC_UNROLL keys per group in flight, a per-group online softmax in fp32 (exp2 domain), the lane-exchange
// merge, the LDS merge in wave order, the same fp32 partials (acc[hs], m, l) — so the combine launch, the workspace and the split rule
// are obte_attn_decode's.  KV8_DPL dims (= code bytes) per lane and key, hs / KV8_DPL lanes per key.  The key's scale multiplies the score
// after the group sum (scale * log2 e stays folded into q), the value's scale the probability used for P V, l sums the unscaled
// probability.  The tail rule covers the scales: a key at or beyond k1 has its code loads AND its scale loads redirected to the split's
// last key, its score is -inf, its weight an exact 0 and its V a selected 0.
#include "common.h"

#ifndef KV8_DPL
#define KV8_DPL 16   // 8 or 16 (DESIGN.md 14.7 has both register reports and the measurement that chose)
#endif

namespace {

// OP over every aligned group of LPR (4, 8 or 16) consecutive lanes, the result on each lane of the group (group_sum's steps)
template <int LPR, bool MAX>
__device__ __forceinline__ float group_reduce(float v) {
    auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : a + b; };
    v = op(v, dpp_moved<0xB1>(v));                        // quad_perm [1,0,3,2]
    v = op(v, dpp_moved<0x4E>(v));                        // quad_perm [2,3,0,1]
    if (LPR >= 8) v = op(v, dpp_moved<0x141>(v));         // row_half_mirror: 8 lanes
    if (LPR == 16) v = op(v, dpp_moved<0x140>(v));        // row_mirror: 16 lanes
    return v;
}

// ---- the store ------------------------------------------------------------------------------------------------------------------------------
// One thread per 16 bytes of the packed qkv.  ROPE = false (obte_kv8_cache_store): item = ((row * 2 + which) * C + column) / 8 of the k and v
// thirds of the rotated rows row = b t + ti, stored at position pos0 + ti.  ROPE = true (obte_kv8_cache_rope_store_rows): item = ((row * 3 +
// third) * C + column) / 8 of the unrotated row b at position pos[b] (outside [0, max_pos]: the row is left alone), its q and k thirds rotated
// in place.  A head's hs / 8 items are consecutive lanes of one wave (C / 8 and 256 are multiples of hs / 8), all of them in or all out.
// n_vec = B H T_max: the V codes lie n_vec hs bytes behind the K codes, the K scales 2 n_vec hs bytes, the V scales 4 n_vec more.
template <bool ROPE>
__global__ __launch_bounds__(256) void kv8_store_kernel(bf16* __restrict__ qkv, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                        const int32_t* __restrict__ pos, int max_pos, uint8_t* __restrict__ cache, int64_t items, int t,
                                                        int H, int hs, int64_t T_max, int64_t pos0, int64_t n_vec) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    constexpr int THIRDS = ROPE ? 3 : 2;
    const int C = H * hs, cpr = C / 8;
    const int c8 = (int)(i % cpr);
    const int64_t rw = i / cpr;
    const int third = (int)(rw % THIRDS) + (ROPE ? 0 : 1);   // 0 q, 1 k, 2 v
    const int64_t row = rw / THIRDS;
    int64_t b, p;
    if (ROPE) {
        b = row;
        const int p0 = pos[b];
        if (p0 < 0 || p0 > max_pos) return;
        p = p0;
    } else {
        b = row / t;
        p = pos0 + row % t;
    }
    const int col = c8 * 8, h = col / hs, e = col % hs;
    bf16* ptr = qkv + row * 3 * C + (int64_t)third * C + col;
    bf16x8 v = *reinterpret_cast<const bf16x8*>(ptr);
    if (ROPE && third < 2) {   // the arithmetic of OBTE_EPI_ROPE_QK and of kv_cache_rope_store_chunk_kernel
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
    if (third == 0) return;   // (uniform over a head's lanes)
    float f[8], amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        f[j] = bf2f(v[j]);
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
    const int which = third - 1;
    const int64_t vec = (b * H + h) * T_max + p;   // the head vector's index in [B, H, T_max]
    *reinterpret_cast<u32x2*>(cache + (which * n_vec + vec) * hs + e) = u32x2{(uint32_t)w0, (uint32_t)w1};
    if (e == 0) reinterpret_cast<float*>(cache + 2 * n_vec * hs)[which * n_vec + vec] = __builtin_bit_cast(float, (uint32_t)(ex + 127) << 23);
}

// ---- the attention --------------------------------------------------------------------------------------------------------------------------
template <int DPL>
struct Part8 { float m, l, acc[DPL]; };   // one online-softmax state, exp2 domain, for the DPL dims of a lane

// a += b with both rescaled to the common maximum; an empty side (m = -inf, l = 0, acc = 0) adds exactly nothing
template <int DPL>
__device__ __forceinline__ void merge8(Part8<DPL>& a, const Part8<DPL>& b) {
    const float m = fmaxf(a.m, b.m);
    const float ms = m == -INFINITY ? 0.f : m;
    const float wa = __builtin_amdgcn_exp2f(a.m - ms), wb = __builtin_amdgcn_exp2f(b.m - ms);
    a.m = m;
    a.l = a.l * wa + b.l * wb;
#pragma unroll
    for (int j = 0; j < DPL; ++j) a.acc[j] = a.acc[j] * wa + b.acc[j] * wb;
}

// DPL / 4 words of codes -> DPL floats (v_cvt_pk_f32_fp8: two of a word's four bytes at a time)
template <int DPL>
__device__ __forceinline__ void decode8(const uint32_t* w, float* f) {
    typedef __attribute__((ext_vector_type(2))) float f32x2;
#pragma unroll
    for (int j = 0; j < DPL / 4; ++j) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
        f[4 * j] = lo[0]; f[4 * j + 1] = lo[1]; f[4 * j + 2] = hi[0]; f[4 * j + 3] = hi[1];
    }
}

template <int DPL>
struct Codes { uint32_t w[DPL / 4]; };
template <int DPL>
__device__ __forceinline__ Codes<DPL> load_codes(const uint8_t* p) {
    Codes<DPL> c;
    if (DPL == 16) {
        const u32x4 r = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
        for (int j = 0; j < DPL / 4; ++j) c.w[j] = r[j];
    } else {
        const u32x2 r = *reinterpret_cast<const u32x2*>(p);
        c.w[0] = r[0]; c.w[1] = r[1];
    }
    return c;
}

// DEC_UNROLL keys of one lane group.  TAIL: some of them may lie at or beyond k1.
template <int HS, int DPL, bool TAIL>
__device__ __forceinline__ void decode_keys8(Part8<DPL>& st, const float* qf, const uint8_t* kb, const uint8_t* vb, const float* ks, const float* vs, int key0,
                                             int kstride, int k1, int chunk) {
    constexpr int LPR = HS / DPL;
    Codes<DPL> kr[DEC_UNROLL], vr[DEC_UNROLL];
    float ksc[DEC_UNROLL], vsc[DEC_UNROLL];
    bool ok[DEC_UNROLL];
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
        const int key = key0 + u * kstride;
        ok[u] = !TAIL || key < k1;
        const int64_t kk = ok[u] ? key : k1 - 1;   // (k1 - 1 >= k0: a workgroup with no key never gets here)
        kr[u] = load_codes<DPL>(kb + kk * HS + chunk * DPL);
        vr[u] = load_codes<DPL>(vb + kk * HS + chunk * DPL);
        ksc[u] = ks[kk];
        vsc[u] = vs[kk];
    }
    float sc[DEC_UNROLL];
    float mx = st.m;
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
        float kf[DPL];
        decode8<DPL>(kr[u].w, kf);
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < DPL; ++j) d = __builtin_fmaf(qf[j], kf[j], d);
        d = group_reduce<LPR, false>(d) * ksc[u];
        sc[u] = ok[u] ? d : -INFINITY;
        mx = fmaxf(mx, sc[u]);
    }
    const float ms = (TAIL && mx == -INFINITY) ? 0.f : mx;
    const float alpha = __builtin_amdgcn_exp2f(st.m - ms);
    st.m = mx;
    st.l *= alpha;
#pragma unroll
    for (int j = 0; j < DPL; ++j) st.acc[j] *= alpha;
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
        const float p = ok[u] ? __builtin_amdgcn_exp2f(sc[u] - ms) : 0.f;
        const float pv = p * vsc[u];
        Codes<DPL> vz = vr[u];
        if (TAIL && !ok[u]) {
#pragma unroll
            for (int j = 0; j < DPL / 4; ++j) vz.w[j] = 0u;
        }
        float vf[DPL];
        decode8<DPL>(vz.w, vf);
        st.l += p;
#pragma unroll
        for (int j = 0; j < DPL; ++j) st.acc[j] = __builtin_fmaf(pv, vf[j], st.acc[j]);
    }
}

// HS: 64 or 128.  grid (splits, B * H), DEC_WAVES * 64 threads.  per: keys per split (a multiple of DEC_CHUNK).  n_vec = B H T_max.
// splits == 1: o and lse are final.  Else part[(bh * splits + split) * (HS + DEC_PAD)] = (acc[HS], m, l): attn_decode_kernel's layout.
// ROWS: row b has rows_n[b] + rows_off keys if that lies in [1, n_keys] (n_keys: the host's bound), else none; per is formed here.
template <int HS, bool ROWS, int DPL>
__global__ __launch_bounds__(DEC_WAVES * 64) void attn_decode_kv8_kernel(const bf16* __restrict__ q, int64_t q_ld, const uint8_t* __restrict__ cache,
                                                                          bf16* __restrict__ o, float* __restrict__ lse, float* __restrict__ part, int H,
                                                                          int64_t T_max, int64_t n_vec, int n_keys, int per, float qscale,
                                                                          const int32_t* __restrict__ rows_n, int rows_off) {
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
    for (int j = 0; j < DPL / 8; ++j) {
        const bf16x8 qv = *reinterpret_cast<const bf16x8*>(q + b * q_ld + h * HS + chunk * DPL + j * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) qf[j * 8 + i] = bf2f(qv[i]) * qscale;
    }

    const uint8_t* kb = cache + (int64_t)bh * T_max * HS;
    const uint8_t* vb = kb + n_vec * HS;
    const float* ks = reinterpret_cast<const float*>(cache + 2 * n_vec * HS) + (int64_t)bh * T_max;
    const float* vs = ks + n_vec;
    Part8<DPL> st;
    st.m = -INFINITY; st.l = 0.f;
#pragma unroll
    for (int j = 0; j < DPL; ++j) st.acc[j] = 0.f;

    constexpr int KSTRIDE = DEC_WAVES * G;              // keys between two of a lane group's DEC_UNROLL keys
    constexpr int ROUND = KSTRIDE * DEC_UNROLL;         // keys of one workgroup round
    const int full_end = k0 + (k1 - k0) / ROUND * ROUND;
    int base = k0;
    for (; base < full_end; base += ROUND) decode_keys8<HS, DPL, false>(st, qf, kb, vb, ks, vs, base + wave * G + grp, KSTRIDE, k1, chunk);
    if (base < k1) decode_keys8<HS, DPL, true>(st, qf, kb, vb, ks, vs, base + wave * G + grp, KSTRIDE, k1, chunk);   // (workgroup-uniform)

    // the lane groups of a wave: exchange with the lane LPR, 2 LPR, .. 32 away (the same dims of another key's state)
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1) {
        Part8<DPL> other;
        other.m = __shfl_xor(st.m, off, 64); other.l = __shfl_xor(st.l, off, 64);
#pragma unroll
        for (int j = 0; j < DPL; ++j) other.acc[j] = __shfl_xor(st.acc[j], off, 64);
        // both partners must add in one order for the result to be the same on each: the lower lane's state first
        if (lane & off) { Part8<DPL> t = other; merge8(t, st); st = t; }
        else merge8(st, other);
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
    Part8<DPL> tot;
    tot.m = lds[0][lane][0]; tot.l = lds[0][lane][1];
#pragma unroll
    for (int j = 0; j < DPL; ++j) tot.acc[j] = lds[0][lane][2 + j];
#pragma unroll
    for (int w = 1; w < DEC_WAVES; ++w) {
        Part8<DPL> p;
        p.m = lds[w][lane][0]; p.l = lds[w][lane][1];
#pragma unroll
        for (int j = 0; j < DPL; ++j) p.acc[j] = lds[w][lane][2 + j];
        merge8(tot, p);
    }
    if (splits == 1) {   // n_keys >= 1: l > 0; an inactive row (ROWS): l = 0, o = 0 and lse = -inf
        const float inv = (ROWS && tot.l == 0.f) ? 0.f : 1.0f / tot.l;
#pragma unroll
        for (int j = 0; j < DPL / 8; ++j) {
            bf16x8 out;
#pragma unroll
            for (int i = 0; i < 8; ++i) out[i] = f2bf(tot.acc[j * 8 + i] * inv);
            *reinterpret_cast<bf16x8*>(o + ((int64_t)bh * HS + lane * DPL + j * 8)) = out;
        }
        if (lse && lane == 0)
            lse[bh] = (ROWS && tot.l == 0.f) ? -INFINITY : (tot.m + __builtin_amdgcn_logf(tot.l)) * 0.6931471805599453f;   // v_log_f32 is log2
        return;
    }
    float* pr = part + ((int64_t)bh * splits + split) * (HS + DEC_PAD);
#pragma unroll
    for (int j = 0; j < DPL / 4; ++j)
        *reinterpret_cast<f32x4*>(pr + lane * DPL + j * 4) = f32x4{tot.acc[4 * j], tot.acc[4 * j + 1], tot.acc[4 * j + 2], tot.acc[4 * j + 3]};
    if (lane == 0) { pr[HS] = tot.m; pr[HS + 1] = tot.l; }
}

bool kv8_shape_ok(int64_t B, int64_t T_max, int32_t n_head, int32_t head_dim) { return obte_kv_cache_bytes(B, T_max, n_head, head_dim) > 0; }

template <int HS, bool ROWS>
void launch_decode_kv8(const dim3& grid, hipStream_t st, const bf16* q, int64_t q_ld, const uint8_t* cache, bf16* o, float* lse, float* ws, int H, int64_t T_max,
                       int64_t n_vec, int n_keys, int per, float qscale, const int32_t* rows_n, int key_off) {
    hipLaunchKernelGGL((attn_decode_kv8_kernel<HS, ROWS, KV8_DPL>), grid, dim3(DEC_WAVES * 64), 0, st, q, q_ld, cache, o, lse, ws, H, T_max, n_vec, n_keys, per, qscale,
                       rows_n, key_off);
    if (grid.x > 1) obte_attn_decode_combine(HS, (int)grid.y, (int)grid.x, ws, o, lse, st);
}

}  // namespace

extern "C" int64_t obte_kv8_cache_bytes(int64_t B, int64_t T_max, int32_t n_head, int32_t head_dim) {
    return kv8_shape_ok(B, T_max, n_head, head_dim) ? 2 * B * n_head * T_max * (int64_t)(head_dim + 4) : 0;
}

extern "C" int obte_kv8_cache_store(const obte_bf16* qkv, int64_t B, int64_t t, int32_t n_head, int32_t head_dim, void* cache8, int64_t T_max, int64_t pos0,
                                    obte_stream s) {
    OBTE_REQUIRE(qkv && cache8, "obte_kv8_cache_store: null pointer");
    OBTE_REQUIRE(kv8_shape_ok(B, T_max, n_head, head_dim), "obte_kv8_cache_store: bad shape (head_dim 64 or 128)");
    OBTE_REQUIRE(t > 0 && pos0 >= 0 && pos0 + t <= T_max, "obte_kv8_cache_store: positions [%lld, %lld) do not fit T_max = %lld", (long long)pos0,
                 (long long)(pos0 + t), (long long)T_max);
    OBTE_REQUIRE((((uintptr_t)qkv | (uintptr_t)cache8) & 15) == 0, "obte_kv8_cache_store: qkv and cache8 must be 16-byte aligned");
    const int64_t items = B * t * 2 * n_head * head_dim / 8;
    OBTE_REQUIRE(cdiv64(items, 256) < (1ll << 31), "obte_kv8_cache_store: too many rows for one launch");
    // (the kernel only reads qkv without ROPE)
    hipLaunchKernelGGL(kv8_store_kernel<false>, dim3((unsigned)cdiv64(items, 256)), dim3(256), 0, (hipStream_t)s, (bf16*)qkv, (const float*)nullptr,
                       (const float*)nullptr, (const int32_t*)nullptr, 0, (uint8_t*)cache8, items, (int)t, n_head, head_dim, T_max, pos0, B * n_head * T_max);
    OBTE_CHECK_LAUNCH("obte_kv8_cache_store");
    return OBTE_OK;
}

// obte_kv8_cache_rope_store_rows behind its checks; who: the entry point named in an error (csrc/block.cpp: obte_block_decode_kv8)
int obte_kv8_rope_store_rows_as(const char* who, obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos, int64_t max_pos, int64_t B,
                                int32_t n_head, int32_t head_dim, void* cache8, int64_t T_max, obte_stream s) {
    OBTE_REQUIRE(qkv && rope_cos && rope_sin && pos && cache8, "%s: null pointer", who);
    OBTE_REQUIRE(kv8_shape_ok(B, T_max, n_head, head_dim), "%s: bad shape (head_dim 64 or 128)", who);
    OBTE_REQUIRE(max_pos >= 0 && max_pos < T_max, "%s: max_pos = %lld outside [0, T_max = %lld)", who, (long long)max_pos, (long long)T_max);
    OBTE_REQUIRE((((uintptr_t)qkv | (uintptr_t)cache8 | (uintptr_t)rope_cos | (uintptr_t)rope_sin) & 15) == 0 && ((uintptr_t)pos & 3) == 0,
                 "%s: qkv, cache8 and the tables must be 16-byte aligned, pos 4-byte aligned", who);
    const int64_t items = B * 3 * n_head * head_dim / 8;
    OBTE_REQUIRE(cdiv64(items, 256) < (1ll << 31), "%s: too many rows for one launch", who);
    hipLaunchKernelGGL(kv8_store_kernel<true>, dim3((unsigned)cdiv64(items, 256)), dim3(256), 0, (hipStream_t)s, (bf16*)qkv, rope_cos, rope_sin, pos, (int)max_pos,
                       (uint8_t*)cache8, items, 1, n_head, head_dim, T_max, (int64_t)0, B * n_head * T_max);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}

extern "C" int obte_kv8_cache_rope_store_rows(obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos, int64_t max_pos, int64_t B,
                                              int32_t n_head, int32_t head_dim, void* cache8, int64_t T_max, obte_stream s) {
    return obte_kv8_rope_store_rows_as("obte_kv8_cache_rope_store_rows", qkv, rope_cos, rope_sin, pos, max_pos, B, n_head, head_dim, cache8, T_max, s);
}

// obte_attn_decode_kv8 with row b's count read as n_keys_rows[b] + key_off (csrc/block.cpp hands a step's positions and 1); the checks and
// the launch of obte_attn_decode / obte_attn_decode_rows (attention_decode.hip, attn_decode_checked) on the e4m3 cache
int obte_attn_decode_kv8_off(const char* who, const obte_bf16* q, int64_t q_ld, const void* cache8, obte_bf16* o, float* lse, int64_t B, int64_t T_max,
                             int64_t n_keys, const int32_t* n_keys_rows, int32_t key_off, int32_t n_head, int32_t head_dim, float scale, int32_t splits, void* ws,
                             int64_t ws_bytes, obte_stream s) {
    const bool rows = n_keys_rows != nullptr;
    OBTE_REQUIRE(q && cache8 && o, "%s: null pointer", who);
    OBTE_REQUIRE(kv8_shape_ok(B, T_max, n_head, head_dim) && B * n_head <= 65535, "%s: bad shape (head_dim 64 or 128, B * n_head <= 65535)", who);
    OBTE_REQUIRE(n_keys >= 1 && n_keys <= T_max, "%s: n_keys = %lld outside [1, T_max = %lld]", who, (long long)n_keys, (long long)T_max);
    OBTE_REQUIRE(q_ld >= (int64_t)n_head * head_dim && q_ld % 8 == 0, "%s: q_ld must be a multiple of 8 and at least n_head * head_dim", who);
    OBTE_REQUIRE((((uintptr_t)q | (uintptr_t)cache8 | (uintptr_t)o) & 15) == 0 && ((uintptr_t)n_keys_rows & 3) == 0,
                 "%s: q, cache8 and o must be 16-byte aligned, n_keys_rows 4-byte aligned", who);
    OBTE_REQUIRE(splits >= 0 && splits <= OBTE_ATTN_DECODE_MAX_SPLITS, "%s: splits = %d outside [0, %d]", who, splits, OBTE_ATTN_DECODE_MAX_SPLITS);
    if (splits == 0) splits = obte_attn_decode_splits(B, n_head, head_dim, n_keys);
    if (splits > 1) {
        const int64_t need = B * n_head * splits * (int64_t)(head_dim + DEC_PAD) * 4;
        OBTE_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0, "%s: %d splits need a 16-byte aligned workspace of %lld bytes, got %lld", who, splits,
                     (long long)need, (long long)(ws ? ws_bytes : 0));
    }
    const int per = rows ? 0 : (int)(cdiv64(cdiv64(n_keys, splits), DEC_CHUNK) * DEC_CHUNK);
    const hipStream_t st = (hipStream_t)s;
    const int BH = (int)(B * n_head);
    const float qscale = scale * 1.4426950408889634f;
    const int64_t n_vec = B * n_head * T_max;
    const int prof = obte_prof_begin(st, 105, BH, n_keys, head_dim);   // cache bytes read = 2 * BH * n_keys * (head_dim + 4) (rows: the bound)
    const dim3 grid((unsigned)splits, (unsigned)BH);
    const bf16* qp = (const bf16*)q;
    const uint8_t* cp = (const uint8_t*)cache8;
    if (head_dim == 128) {
        if (rows) launch_decode_kv8<128, true>(grid, st, qp, q_ld, cp, (bf16*)o, lse, (float*)ws, n_head, T_max, n_vec, (int)n_keys, per, qscale, n_keys_rows, key_off);
        else launch_decode_kv8<128, false>(grid, st, qp, q_ld, cp, (bf16*)o, lse, (float*)ws, n_head, T_max, n_vec, (int)n_keys, per, qscale, nullptr, 0);
    } else {
        if (rows) launch_decode_kv8<64, true>(grid, st, qp, q_ld, cp, (bf16*)o, lse, (float*)ws, n_head, T_max, n_vec, (int)n_keys, per, qscale, n_keys_rows, key_off);
        else launch_decode_kv8<64, false>(grid, st, qp, q_ld, cp, (bf16*)o, lse, (float*)ws, n_head, T_max, n_vec, (int)n_keys, per, qscale, nullptr, 0);
    }
    obte_prof_end(prof, st);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}

extern "C" int obte_attn_decode_kv8(const obte_bf16* q, int64_t q_ld, const void* cache8, obte_bf16* o, float* lse, int64_t B, int64_t T_max, int64_t n_keys,
                                    const int32_t* n_keys_rows, int32_t n_head, int32_t head_dim, float scale, int32_t splits, void* ws, int64_t ws_bytes,
                                    obte_stream s) {
    return obte_attn_decode_kv8_off("obte_attn_decode_kv8", q, q_ld, cache8, o, lse, B, T_max, n_keys, n_keys_rows, 0, n_head, head_dim, scale, splits, ws, ws_bytes, s);
}
