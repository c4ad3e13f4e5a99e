// Weight-streaming product for 1 <= M <= 64 (include/omnibiote_hip_small_m.h): D[M, N] = epilogue(bf16(alpha * x[M, K] W[N, K]^T)), the x W^T
// layout only.  The products of a decode step and the last-position readout run at M = batch: the 256-row tile structures spend them
// on a handful of tiles that are padding, while the work is the one read of W.  Here that read is the kernel:
//   - grid ceil(N / 16): a workgroup of SM_WAVES waves owns one strip of 16 rows of W, every byte of which is loaded exactly once, 16
//     bytes per lane, global -> VGPR, as the v_mfma_f32_16x16x32_bf16 fragment it is (lane l: row l & 15, k = 8 (l >> 4) + j).  No LDS
//     staging of W.  The two 32-deep k-steps of a 64-deep chunk are loaded back to back, so the wave that touches a 128-byte line of a
//     row consumes the whole of it.
//   - K is split over the waves in 64-deep chunks, chunk c to wave c % SM_WAVES (neighbouring waves read neighbouring lines); a wave
//     keeps the W loads of UNR chunks (2 UNR KiB) in flight before it uses the first.  A wave whose share is empty (K < 64 SM_WAVES)
//     carries zeros.
//   - x: rows 16 i .. 16 i + 15 are the other operand of MFMA i (MT = ceil(M / 16) of them per W fragment, the same fragment shape,
//     from L2); a row index >= M is clamped to M - 1 and its result never leaves the workgroup.  Row r of the result is column r of an
//     MFMA: it depends on x[r] and W alone.
//   - the waves' fp32 partials meet in LDS and are summed in wave order.  Chunk order within a wave and wave order across them are
//     functions of K only: row m has the same bits at every M, and in every call.
//   - one thread per (row, 8 columns): bf16(alpha * sum), then the epilogue in the arithmetic of the tile structures' tile_epilogue
//     (gemm_bf16_v2.hip) on the rounded value, one 16-byte store.  Columns >= N (the half strip of N % 16 == 8) and rows >= M are
//     never written; their W rows are clamped to N - 1 on the way in.
// No cross-workgroup split of K: N = C launches N / 16 workgroups (64 at C = 1024) and are bound by the launch, not by the stream.
// A second kernel with the same arithmetic, small_m_xs_kernel below, serves many strips over a short K (the readout) with x held in
// registers; which of the two runs is a function of (N, K).  Measurements and register figures: DESIGN.md 14.2.
// The format of W is a policy of both kernels (WBf16 / WE4m3 below, as attention_decode.hip has CacheBf16 / CacheE4m3): W as OCP e4m3 codes
// with one power-of-two fp32 scale per row (include/omnibiote_hip_w8.h, obte_linear_small_m_w8) is the same kernels with half the bytes per
// lane, an exact code -> bf16 conversion in front of the same MFMA and the row's scale on the fp32 sum in the finish.  DESIGN.md 14.11.
// WMxfp4: W as OCP MXFP4 (include/omnibiote_hip_w4.h, obte_linear_small_m_w4), a quarter of the bytes per lane and one scale byte per 32-deep
// block, applied inside the exact conversion: nothing reaches the finish.  DESIGN.md 14.20.
#include "common.h"
#include <atomic>
#include <stdlib.h>

namespace {

constexpr int SM_WAVES = 4;
constexpr int SM_MAX_M = 64;

struct SmallMParams {
    const bf16* x; const bf16* w; bf16* d; const bf16* aux;
    int64_t N, lda, ldb, ldd;
    int M, K;
    float alpha;
    const float* rope_cos; const float* rope_sin; uint32_t rope_T, rope_hs;
};

struct SmallMParamsW8 : SmallMParams {   // w is null, ldb the codes' row stride in bytes
    const uint8_t* codes; const float* scales;
};

struct SmallMParamsW4 : SmallMParams {   // w is null, ldb the codes' row stride in bytes, lds the scale bytes'
    const uint8_t* codes; const uint8_t* scales; int64_t lds;
};

// ---- the format of W ---------------------------------------------------------------------------------------------------------------------
// Row: a lane's pointer into row n of W (lane group fq); Raw: what the lane loads for one 64-deep chunk, both 32-deep k-steps; frag(raw, s): the
// bf16 MFMA fragment of k-step s; Scale: what a finishing thread holds for its 8 columns, applied to the fp32 sums before alpha.
struct WBf16 {
    using Params = SmallMParams;
    using Row = const bf16*;
    struct Raw { bf16x8 f[2]; };
    struct Scale {};
    static constexpr const char* NAME = "obte_linear_small_m_bf16";
    static __device__ __forceinline__ Row row(const Params& p, int64_t n, int fq) { return p.w + n * p.ldb + fq * 8; }
    static __device__ __forceinline__ Raw load(Row r, int64_t k) {
        Raw w;
#pragma unroll
        for (int s = 0; s < 2; ++s) w.f[s] = *reinterpret_cast<const bf16x8*>(r + k + s * 32);
        return w;
    }
    static __device__ __forceinline__ bf16x8 frag(const Raw& w, int s) { return w.f[s]; }
    static __device__ __forceinline__ Scale scale(const Params&, int64_t, bool) { return {}; }
    static __device__ __forceinline__ void apply(f32x4&, f32x4&, const Scale&) {}
};
// e4m3 codes, 64 to a chunk in the order pack_codes (omnibiote_amd/w8quant.py) leaves them: byte 16 fq + 8 s + j of a 64-byte group is the code
// of k = 32 s + 8 fq + j, so a lane's two fragments are ONE 16-byte load.  A code becomes its bf16 exactly: an e4m3 value has at most 4
// significant bits and an exponent inside bf16's range, so the upper half of v_cvt_pk_f32_fp8's fp32 is the bf16 (the instruction
// attention_decode.hip reads its cache with; v_cvt_scalef32_pk_bf16_fp8 would halve these 8 + 8 VALU operations per chunk, which a kernel
// bound by its loads does not feel, and its scale operand's behaviour is documented less plainly).
struct WE4m3 {
    using Params = SmallMParamsW8;
    using Row = const uint8_t*;
    struct Raw { u32x4 q; };
    struct Scale { float v[8]; };
    static constexpr const char* NAME = "obte_linear_small_m_w8";
    static __device__ __forceinline__ Row row(const Params& p, int64_t n, int fq) { return p.codes + n * p.ldb + fq * 16; }
    static __device__ __forceinline__ Raw load(Row r, int64_t k) { return Raw{*reinterpret_cast<const u32x4*>(r + k)}; }
    static __device__ __forceinline__ bf16x8 frag(const Raw& w, int s) {
        typedef __attribute__((ext_vector_type(2))) float f32x2;
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int word = (int)w.q[2 * s + j];
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(word, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(word, true);
            // v_perm_b32: the upper halves of two fp32, the first in the low half (bytes 2, 3 of the second operand, then 6, 7 = bytes 2, 3 of the
            // first).  The elements are copied out first: __builtin_bit_cast applied to lo[1] itself read element 0 of the vector.
            const float f0 = lo[0], f1 = lo[1], f2 = hi[0], f3 = hi[1];
            o[2 * j] = __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, f1), __builtin_bit_cast(uint32_t, f0), 0x07060302u);
            o[2 * j + 1] = __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, f3), __builtin_bit_cast(uint32_t, f2), 0x07060302u);
        }
        return __builtin_bit_cast(bf16x8, o);
    }
    // columns n .. n + 7 (n % 8 == 0, and N % 8 == 0: all below N when n is); scales is 4-byte aligned only
    static __device__ __forceinline__ Scale scale(const Params& p, int64_t n, bool mine) {
        Scale sc;
#pragma unroll
        for (int j = 0; j < 8; ++j) sc.v[j] = mine ? p.scales[n + j] : 0.f;
        return sc;
    }
    static __device__ __forceinline__ void apply(f32x4& lo, f32x4& hi, const Scale& sc) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { lo[j] *= sc.v[j]; hi[j] *= sc.v[4 + j]; }
    }
};
// MXFP4 (include/omnibiote_hip_w4.h): OCP e2m1 codes, two to a byte, 32 bytes to a chunk in the order pack_codes (omnibiote_amd/w4quant.py)
// leaves them — byte 8 fq + 4 s + j / 2 of a 32-byte group holds k = 32 s + 8 fq + j, even j in the low nibble — so a lane's two fragments
// are ONE 8-byte load, word s the eight codes of k-step s in k order; and one e8m0 byte per 32-deep block of a row, which is one k-step of
// one row: the two of a chunk are one 2-byte load, every lane of a row the same two.  v_cvt_scalef32_pk_bf16_fp4 turns byte `sel` of a word
// into two bf16 (the low nibble first) times 2^(exponent field of the scale operand - 127); the operand here is the fp32 with the e8m0 byte as its
// exponent field and no mantissa, 2^(byte - 127) itself for the bytes 1 .. 254.  An e2m1 value has 2 significant bits and the quantiser's
// scales keep every product a normal bf16, so the conversion is exact and the block's scale needs no place in the sum: Scale is empty.
struct WMxfp4 {
    using Params = SmallMParamsW4;
    struct Row { const uint8_t* c; const uint8_t* e; };
    struct Raw { u32x2 q; uint32_t e; };
    struct Scale {};
    static constexpr const char* NAME = "obte_linear_small_m_w4";
    static __device__ __forceinline__ Row row(const Params& p, int64_t n, int fq) { return Row{p.codes + n * p.ldb + fq * 8, p.scales + n * p.lds}; }
    static __device__ __forceinline__ Raw load(Row r, int64_t k) {   // k % 64 == 0
        return Raw{*reinterpret_cast<const u32x2*>(r.c + (k >> 1)), *reinterpret_cast<const uint16_t*>(r.e + (k >> 5))};
    }
    static __device__ __forceinline__ bf16x8 frag(const Raw& w, int s) {
        const float scale = __builtin_bit_cast(float, ((w.e >> (8 * s)) & 0xffu) << 23);
        const uint32_t word = w.q[s];
        const bf16x2 f0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 0), f1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 1);
        const bf16x2 f2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 2), f3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 3);
        return bf16x8{f0[0], f0[1], f1[0], f1[1], f2[0], f2[1], f3[0], f3[1]};
    }
    static __device__ __forceinline__ Scale scale(const Params&, int64_t, bool) { return {}; }
    static __device__ __forceinline__ void apply(f32x4&, f32x4&, const Scale&) {}
};
// the thread of small_m_finish that owns columns n .. n + 7 of a strip at n0 loads their scales ahead of the sum
template <class WF, int MT>
__device__ __forceinline__ typename WF::Scale small_m_scale(const typename WF::Params& p, int64_t n0) {
    const int t = threadIdx.x;
    const int64_t n = n0 + (t & 1) * 8;
    return WF::scale(p, n, t < MT * 32 && (t >> 1) < p.M && n < p.N);
}

template <class WF, int MT, int UNR>
__device__ __forceinline__ void small_m_chunks(f32x4 (&acc)[MT], typename WF::Row wrow, const bf16* const (&xrow)[MT], int64_t k0) {
    typename WF::Raw wf[UNR];
    bf16x8 xf[UNR][2][MT];
#pragma unroll
    for (int u = 0; u < UNR; ++u) wf[u] = WF::load(wrow, k0 + u * (SM_WAVES * 64));
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < MT; ++i) xf[u][s][i] = *reinterpret_cast<const bf16x8*>(xrow[i] + k0 + u * (SM_WAVES * 64) + s * 32);
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bf16x8 wfr = WF::frag(wf[u], s);
#pragma unroll
            for (int i = 0; i < MT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr, xf[u][s][i], acc[i], 0, 0, 0);
        }
}

// The rotation of tile_epilogue (gemm_bf16_v2.hip), xe c - xo s and xe s + xo c, in the contracted form hipcc gives that expression
// there — the first product fused into the sum, the second rounded on its own — spelled out, so that both kernels below and the tile
// structures agree bit for bit whatever surrounds the expression (left to the compiler, the two kernels here contracted it differently)
__device__ __forceinline__ float rope_even(float xe, float xo, float c, float s) {
#pragma clang fp contract(off)
    const float t = xo * s;
    return __builtin_fmaf(xe, c, -t);
}
__device__ __forceinline__ float rope_odd(float xe, float xo, float c, float s) {
#pragma clang fp contract(off)
    const float t = xo * c;
    return __builtin_fmaf(xe, s, t);
}

// One thread per (row r, 8 columns) of a 16-column strip at n0: the waves' partials summed in wave order, bf16(alpha * sum), the epilogue
// on the rounded value (tile_epilogue's arithmetic, gemm_bf16_v2.hip), one 16-byte store
template <class WF, int MT, int EPI>
__device__ __forceinline__ void small_m_finish(const typename WF::Params& p, const float (&red)[SM_WAVES][MT * 16][16], int64_t n0, const typename WF::Scale& sc) {
    const int t = threadIdx.x;
    const int r = t >> 1, half = t & 1;
    const int64_t n = n0 + half * 8;
    if (t >= MT * 32 || r >= p.M || n >= p.N) return;
    f32x4 lo = *reinterpret_cast<const f32x4*>(&red[0][r][half * 8]), hi = *reinterpret_cast<const f32x4*>(&red[0][r][half * 8 + 4]);
#pragma unroll
    for (int w = 1; w < SM_WAVES; ++w) {
        lo += *reinterpret_cast<const f32x4*>(&red[w][r][half * 8]);
        hi += *reinterpret_cast<const f32x4*>(&red[w][r][half * 8 + 4]);
    }
    WF::apply(lo, hi, sc);   // e4m3: the row's scale, before alpha
    const bf16x4 vlo = __builtin_convertvector(lo * p.alpha, bf16x4), vhi = __builtin_convertvector(hi * p.alpha, bf16x4);
    bf16x8 v = join8(vlo, vhi);
    const int64_t o = (int64_t)r * p.ldd + n;
    if (EPI == OBTE_EPI_GELU_ACT) {
        v = gelu_act8(v);
    } else if (EPI == OBTE_EPI_ADD) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(p.aux + o);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = f2bf(bf2f(a[j]) + bf2f(v[j]));
    } else if (EPI == OBTE_EPI_ROPE_QK) {
        if (n < 2 * (p.N / 3)) {   // the q and k thirds; position = row % T (tile_epilogue's expression)
            const uint32_t mu = (uint32_t)r, nu = (uint32_t)n, T32 = p.rope_T, hs32 = p.rope_hs;
            const uint32_t tt = (T32 & (T32 - 1)) == 0 ? (mu & (T32 - 1)) : (mu % T32);
            const uint32_t dd = (hs32 & (hs32 - 1)) == 0 ? (nu & (hs32 - 1)) : (nu % hs32);
            const f32x4 cs = *reinterpret_cast<const f32x4*>(p.rope_cos + tt * (hs32 / 2) + dd / 2);
            const f32x4 sn = *reinterpret_cast<const f32x4*>(p.rope_sin + tt * (hs32 / 2) + dd / 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xe = bf2f(v[2 * j]), xo = bf2f(v[2 * j + 1]);
                v[2 * j] = f2bf(rope_even(xe, xo, cs[j], sn[j]));
                v[2 * j + 1] = f2bf(rope_odd(xe, xo, cs[j], sn[j]));
            }
        }
    }
    *reinterpret_cast<bf16x8*>(p.d + o) = v;
}

// The same product with x stationary, for many strips over a short K (the readout: N = vocabulary, K = C; K = 256, 512 or 1024, that
// is CH = 1, 2 or 4 chunks per wave).  With one strip per workgroup every strip re-reads its M x K of x from L2 in
// fragment-shaped pieces (16 rows x 64 B per instruction), 4 x the bytes of the strip's W at M = 64: the readout ran at 0.27 of the HBM rate.
// Here a wave loads its whole share of x once (MT x K / 256 fragment pairs: 128 VGPRs at M = 64, K = 1024) and the workgroup walks spw
// consecutive strips against it; the W fragments of strip s + 1 are in flight under the MFMAs, the reduction and the stores of strip s
// (two LDS buffers, one barrier per strip).  Chunk order, wave order and the finish are small_m_kernel's: the same bits.
constexpr int SM_XS_GRID = 512;   // workgroups the strips are dealt to: two per CU, all resident

template <class WF, int MT, int EPI, int CH>
__global__ __launch_bounds__(SM_WAVES * 64) void small_m_xs_kernel(const typename WF::Params p, int spw) {
    __shared__ float red[2][SM_WAVES][MT * 16][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    // CH = K / 256 chunks per wave (a template argument: a run-time count put a branch around every load): chunk c of this wave is chunk
    // wave + c SM_WAVES of the row
    const int64_t strips = (p.N + 15) / 16;
    const int64_t s0 = (int64_t)blockIdx.x * spw, s1 = min(s0 + spw, strips);

    bf16x8 xf[CH][2][MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const bf16* xrow = p.x + (int64_t)min(i * 16 + fr, p.M - 1) * p.lda + fq * 8 + wave * 64;
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int s = 0; s < 2; ++s) xf[c][s][i] = *reinterpret_cast<const bf16x8*>(xrow + c * (SM_WAVES * 64) + s * 32);
    }
    auto load_w = [&](typename WF::Raw (&wf)[CH], int64_t strip) {
        const typename WF::Row wrow = WF::row(p, min(strip * 16 + fr, p.N - 1), fq);
#pragma unroll
        for (int c = 0; c < CH; ++c) wf[c] = WF::load(wrow, (wave + c * SM_WAVES) * 64);
    };
    typename WF::Raw wf[CH], wn[CH] = {};
    // (e4m3) the scales of a strip travel with its W: issued ahead of it, so that the finish's wait for them leaves the next strip's W in flight
    typename WF::Scale sc = small_m_scale<WF, MT>(p, s0 * 16), sn = {};
    load_w(wf, s0);
    // x and the first strip have landed before the loop (the first MFMAs need all of them anyway): stated here, the loop's own counted
    // waits cover W alone and strip s + 1 stays in flight across the barrier; left to the loop, hipcc waited vmcnt(0) for x in every pass
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    for (int64_t strip = s0; strip < s1; ++strip) {
        if (strip + 1 < s1) { sn = small_m_scale<WF, MT>(p, (strip + 1) * 16); load_w(wn, strip + 1); }
        f32x4 acc[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 wfr = WF::frag(wf[c], s);
#pragma unroll
                for (int i = 0; i < MT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr, xf[c][s][i], acc[i], 0, 0, 0);
            }
        const int buf = (int)(strip - s0) & 1;   // strip s + 2 reuses strip s's buffer behind the barrier of strip s + 1, which every reader of s has passed
#pragma unroll
        for (int i = 0; i < MT; ++i) *reinterpret_cast<f32x4*>(&red[buf][wave][i * 16 + fr][fq * 4]) = acc[i];
        __syncthreads();
        small_m_finish<WF, MT, EPI>(p, red[buf], strip * 16, sc);
#pragma unroll
        for (int c = 0; c < CH; ++c) wf[c] = wn[c];
        sc = sn;
    }
}

// grid ceil(N / 16), SM_WAVES * 64 threads, MT * SM_WAVES * 1 KiB of LDS
template <class WF, int MT, int EPI>
__global__ __launch_bounds__(SM_WAVES * 64) void small_m_kernel(const typename WF::Params p) {
    constexpr int UNR = MT <= 2 ? 4 : 2;   // chunks whose loads are in flight together: 2 UNR (1 + MT) 16-byte loads per lane
    __shared__ float red[SM_WAVES][MT * 16][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * 16;
    const int fr = lane & 15, fq = lane >> 4;

    const int64_t wn = min(n0 + fr, p.N - 1);
    const typename WF::Row wrow = WF::row(p, wn, fq);
    const typename WF::Scale sc = small_m_scale<WF, MT>(p, n0);
    const bf16* xrow[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) xrow[i] = p.x + (int64_t)min(i * 16 + fr, p.M - 1) * p.lda + fq * 8;

    f32x4 acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    // this wave's chunks: wave, wave + SM_WAVES, ... < K / 64, in ascending order whatever the batching
    const int nc = p.K / 64;
    const int mine = nc > wave ? (nc - wave + SM_WAVES - 1) / SM_WAVES : 0;
    int c = 0;
    for (; c + UNR <= mine; c += UNR) small_m_chunks<WF, MT, UNR>(acc, wrow, xrow, (int64_t)(wave + c * SM_WAVES) * 64);
    for (; c < mine; ++c) small_m_chunks<WF, MT, 1>(acc, wrow, xrow, (int64_t)(wave + c * SM_WAVES) * 64);

    // lane (fr, fq) of MFMA i holds row 16 i + fr of the result, columns 4 fq .. 4 fq + 3 of the strip
#pragma unroll
    for (int i = 0; i < MT; ++i) *reinterpret_cast<f32x4*>(&red[wave][i * 16 + fr][fq * 4]) = acc[i];
    __syncthreads();

    small_m_finish<WF, MT, EPI>(p, red, n0, sc);
}

template <class WF, int MT, int EPI>
int launch_form(const typename WF::Params& p, hipStream_t st) {
    const int64_t strips = cdiv64(p.N, 16);
    const dim3 block(SM_WAVES * 64);
    // which kernel: a function of (N, K) alone, as is everything that orders a sum (which this choice does not)
    const int ch = p.K % (SM_WAVES * 64) == 0 ? p.K / (SM_WAVES * 64) : 0;
    if (strips > SM_XS_GRID && (ch == 1 || ch == 2 || ch == 4)) {
        const int spw = (int)cdiv64(strips, SM_XS_GRID);
        const dim3 grid((unsigned)cdiv64(strips, spw));
        if (ch == 1) hipLaunchKernelGGL((small_m_xs_kernel<WF, MT, EPI, 1>), grid, block, 0, st, p, spw);
        else if (ch == 2) hipLaunchKernelGGL((small_m_xs_kernel<WF, MT, EPI, 2>), grid, block, 0, st, p, spw);
        else hipLaunchKernelGGL((small_m_xs_kernel<WF, MT, EPI, 4>), grid, block, 0, st, p, spw);
    } else {
        hipLaunchKernelGGL((small_m_kernel<WF, MT, EPI>), dim3((unsigned)strips), block, 0, st, p);
    }
    OBTE_CHECK_LAUNCH(WF::NAME);
    return OBTE_OK;
}
template <class WF, int MT>
int launch_mt(const typename WF::Params& p, int epi, hipStream_t st) {
    switch (epi) {
        case OBTE_EPI_NONE: return launch_form<WF, MT, OBTE_EPI_NONE>(p, st);
        case OBTE_EPI_ADD: return launch_form<WF, MT, OBTE_EPI_ADD>(p, st);
        case OBTE_EPI_GELU_ACT: return launch_form<WF, MT, OBTE_EPI_GELU_ACT>(p, st);
        default: return launch_form<WF, MT, OBTE_EPI_ROPE_QK>(p, st);
    }
}

// the largest M at which the decode sequence takes this product; OBTE_SMALL_M=0 in the environment: 0 from the start
constexpr int SM_DEFAULT_MAX = 64;
std::atomic<int> g_small_m_max{[] { const char* e = getenv("OBTE_SMALL_M"); return (e && e[0] == '0' && !e[1]) ? 0 : SM_DEFAULT_MAX; }()};

}  // namespace

extern "C" int obte_small_m_max(void) { return g_small_m_max.load(std::memory_order_relaxed); }
extern "C" int obte_small_m_max_set(int m) {
    OBTE_REQUIRE(m >= 0 && m <= SM_MAX_M, "obte_small_m_max_set: %d outside 0..%d", m, SM_MAX_M);
    return g_small_m_max.exchange(m, std::memory_order_relaxed);
}

namespace {

// what both formats ask of g (who: the entry point; w8: g->b / ldb are not looked at)
int check_args(const char* who, const obte_gemm_args* g, bool w8) {
    OBTE_REQUIRE(g && g->a && (w8 || g->b) && g->d, "%s: null pointer", who);
    OBTE_REQUIRE(g->M >= 1 && g->M <= SM_MAX_M && g->N > 0 && g->K > 0, "%s: M must be 1..%d, N and K positive (M=%lld N=%lld K=%lld)", who, SM_MAX_M,
                 (long long)g->M, (long long)g->N, (long long)g->K);
    if (!g->a_kmajor || !g->b_kmajor) {
        obte_set_error("%s: the x W^T layout only (a_kmajor = b_kmajor = 1)", who);
        return OBTE_EUNSUPPORTED;
    }
    if (g->epilogue != OBTE_EPI_NONE && g->epilogue != OBTE_EPI_ADD && g->epilogue != OBTE_EPI_GELU_ACT && g->epilogue != OBTE_EPI_ROPE_QK) {
        obte_set_error("%s: epilogue %d is not one of NONE, ADD, GELU_ACT, ROPE_QK", who, g->epilogue);
        return OBTE_EUNSUPPORTED;
    }
    OBTE_REQUIRE(g->K % 64 == 0 && g->K < (1ll << 31), "%s: K %% 64 == 0 (K=%lld)", who, (long long)g->K);
    OBTE_REQUIRE(g->lda % 8 == 0 && (w8 || g->ldb % 8 == 0) && g->ldd % 8 == 0 && g->N % 8 == 0, "%s: lda/ldb/ldd/N must be multiples of 8 (16-byte rows)", who);
    OBTE_REQUIRE(g->lda >= g->K && (w8 || g->ldb >= g->K) && g->ldd >= g->N, "%s: leading dimension too small", who);
    OBTE_REQUIRE(cdiv64(g->N, 16) < (1ll << 31), "%s: N too large", who);
    if (g->epilogue == OBTE_EPI_ADD) OBTE_REQUIRE(g->aux, "%s: EPI_ADD needs aux", who);
    if (g->epilogue == OBTE_EPI_ROPE_QK)
        OBTE_REQUIRE(g->rope_cos && g->rope_sin && g->rope_T > 0 && g->rope_T < (1ll << 31) && g->rope_head_dim > 0 && g->rope_head_dim % 8 == 0 && g->N % 3 == 0 &&
                         (g->N / 3) % g->rope_head_dim == 0,
                     "%s: EPI_ROPE_QK needs cos/sin tables, T, head_dim %% 8 == 0 and N = 3 * n_head * head_dim", who);
    if (g->epilogue != OBTE_EPI_NONE && g->epilogue != OBTE_EPI_ADD) OBTE_REQUIRE(g->alpha == 1.0f, "%s: alpha != 1 only with EPI_NONE / EPI_ADD", who);
    return OBTE_OK;
}

void fill_params(SmallMParams& p, const obte_gemm_args* g) {
    p.x = (const bf16*)g->a; p.w = (const bf16*)g->b; p.d = (bf16*)g->d; p.aux = (const bf16*)g->aux;
    p.N = g->N; p.lda = g->lda; p.ldb = g->ldb; p.ldd = g->ldd; p.M = (int)g->M; p.K = (int)g->K; p.alpha = g->alpha;
    p.rope_cos = g->rope_cos; p.rope_sin = g->rope_sin; p.rope_T = (uint32_t)g->rope_T; p.rope_hs = (uint32_t)g->rope_head_dim;
}

// profiler record as the tile structures': 4 x layout (x W^T: 3) + epilogue + 1000 x structure, the bf16 product being structure 8, the e4m3 one 9
template <class WF>
int launch_any(const typename WF::Params& p, const obte_gemm_args* g, int structure, hipStream_t st) {
    const int prof = obte_prof_begin(st, 4 * 3 + g->epilogue + 1000 * structure, g->M, g->N, g->K);
    int rc;
    switch ((g->M + 15) / 16) {
        case 1: rc = launch_mt<WF, 1>(p, g->epilogue, st); break;
        case 2: rc = launch_mt<WF, 2>(p, g->epilogue, st); break;
        case 3: rc = launch_mt<WF, 3>(p, g->epilogue, st); break;
        default: rc = launch_mt<WF, 4>(p, g->epilogue, st); break;
    }
    obte_prof_end(prof, st);
    return rc;
}

}  // namespace

extern "C" int obte_linear_small_m_bf16(const obte_gemm_args* g, obte_stream s) {
    const int rc = check_args("obte_linear_small_m_bf16", g, false);
    if (rc != OBTE_OK) return rc;
    SmallMParams p;
    fill_params(p, g);
    return launch_any<WBf16>(p, g, 8, (hipStream_t)s);
}

extern "C" int obte_linear_small_m_w8(const obte_gemm_args* g, const void* codes, int64_t ld_codes, const float* scales, obte_stream s) {
    const char* who = "obte_linear_small_m_w8";
    const int rc = check_args(who, g, true);
    if (rc != OBTE_OK) return rc;
    OBTE_REQUIRE(codes && scales, "%s: null pointer", who);
    OBTE_REQUIRE(ld_codes % 16 == 0 && ld_codes >= g->K, "%s: ld_codes must be a multiple of 16 and at least K (ld_codes=%lld K=%lld)", who, (long long)ld_codes,
                 (long long)g->K);
    OBTE_REQUIRE_ALIGNED(who, codes, "codes", 16);
    OBTE_REQUIRE_ALIGNED(who, scales, "scales", 4);
    SmallMParamsW8 p;
    fill_params(p, g);
    p.w = nullptr; p.ldb = ld_codes; p.codes = (const uint8_t*)codes; p.scales = scales;
    return launch_any<WE4m3>(p, g, 9, (hipStream_t)s);
}

extern "C" int obte_linear_small_m_w4(const obte_gemm_args* g, const void* codes, int64_t ld_codes, const void* scales, int64_t ld_scales, obte_stream s) {
    const char* who = "obte_linear_small_m_w4";
    const int rc = check_args(who, g, true);
    if (rc != OBTE_OK) return rc;
    OBTE_REQUIRE(codes && scales, "%s: null pointer", who);
    OBTE_REQUIRE(ld_codes % 8 == 0 && ld_codes >= g->K / 2, "%s: ld_codes must be a multiple of 8 and at least K / 2 (ld_codes=%lld K=%lld)", who, (long long)ld_codes,
                 (long long)g->K);
    OBTE_REQUIRE(ld_scales % 2 == 0 && ld_scales >= g->K / 32, "%s: ld_scales must be even and at least K / 32 (ld_scales=%lld K=%lld)", who, (long long)ld_scales,
                 (long long)g->K);
    OBTE_REQUIRE_ALIGNED(who, codes, "codes", 8);
    OBTE_REQUIRE_ALIGNED(who, scales, "scales", 2);
    SmallMParamsW4 p;
    fill_params(p, g);
    p.w = nullptr; p.ldb = ld_codes; p.codes = (const uint8_t*)codes; p.scales = (const uint8_t*)scales; p.lds = ld_scales;
    return launch_any<WMxfp4>(p, g, 10, (hipStream_t)s);
}
