// Continuing a filled key/value cache by n new positions per row in one call (include/omnibiote_hip_extend.h): the attention of n queries
// per (batch, head) at positions p .. p + n - 1 over cache positions [0, p + j + 1), causal inside the chunk.  The cache layout is
// attention_decode.hip's: K [B, H, T_max, hs], then V; the rows form's rotate-and-store of a chunk stands there with the other cache stores.
//
// obte_attn_extend:
//   - grid (split, 32-query tile, b H + h), 4 waves.  The keys a query tile can see are [0, p + min(n, 32 (tile + 1))); a split owns a
//     run of them (a multiple of 32 keys), and the workgroup's waves divide the run among themselves in 32-key tiles, wave w taking
//     tiles w, w + 4, ...  Every wave serves the same 32 queries and keeps its own online-softmax state (m, l, O^T) for them.
//   - both products on v_mfma_f32_32x32x16_bf16 in the forward kernel's orientation (attention.hip): S^T = K Q^T with the query on the
//     lane, so a query's statistics live in the lane pair (l, l ^ 32), and the f32 score accumulator, converted to bf16 in registers, is
//     the B operand of O^T += V^T P^T.  K rows go global -> VGPR -> A fragment, 16 bytes per lane; V needs the transposed read and
//     passes through a wave-private LDS region in attn_common.h's tile image (no workgroup barrier inside the loop).  A tile's loads
//     are issued behind the score MFMAs of the tile before it, under that tile's softmax and P V.
//   - a key at or beyond the split's end never enters: its loads are redirected to the split's last key, its V arrives as a selected
//     zero and its score is selected to -inf, so whatever the cache holds past p + n (NaN patterns included) cannot reach a result.  A
//     later position of the same chunk is finite by construction and masked by the score alone; a padding query (j >= n) reads the
//     chunk's last query row and is not stored.
//   - the waves merge through LDS in wave order; the workgroup writes o / lse itself (one split) or an fp32 partial to the workspace,
//     which a second launch combines in split order.  No atomics, no flags.  A wave or a split without any visible key carries
//     (m = -inf, l = 0, O = 0); every merge rescales against a maximum made finite first, so exp2(-inf - -inf) is never formed.
//   - rows form: p is read per row on the device; a value outside [0, pos] makes the row inactive (no cache byte read, zeros, -inf).  A
//     workgroup derives its key range from its own row's position, so a row is partitioned exactly as the uniform call at that position.
//
// obte_attn_extend_paged (include/omnibiote_hip_paged_extend.h): the rows form with the keys in the pages of a pool, a sibling kernel further down.
#include "attn_common.h"

namespace {
using namespace obte_attn;

constexpr int EXT_WAVES = 4;
constexpr int EXT_QT = 32;   // queries per workgroup
constexpr int EXT_KT = 32;   // keys per wave tile; split boundaries are multiples of it

template <int D> struct ExtShape {
    static constexpr int NR = D / 2;                             // O^T accumulator registers per lane
    static constexpr int PART = (NR + 2) * 64;                   // floats of one partial: [NR + 2][64 lanes] = O^T, m, l
    static constexpr int VREG = EXT_KT * 2 * D;                  // bytes of a wave's V tile (and of the output rows' staging)
    static constexpr int MERGE = (EXT_WAVES - 1) * PART * 4;     // bytes of the wave merge (waves 1 .. 3)
    static constexpr int LDS = (MERGE > EXT_WAVES * VREG ? MERGE : EXT_WAVES * VREG) + VREG;
};

template <int D> struct ExtState {
    float m, l;
    f32x16 o[D / 32];
    __device__ __forceinline__ void clear() {
        m = -INFINITY; l = 0.f;
#pragma unroll
        for (int i = 0; i < D / 32; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    }
    // this += (om, ol, oo-through-get) with both rescaled to the common maximum; an empty side adds exactly nothing
    template <typename F>
    __device__ __forceinline__ void merge(float om, float ol, F get) {
        const float mm = fmaxf(m, om);
        const float ms = mm == -INFINITY ? 0.f : mm;
        const float wa = fast_exp2(m - ms), wb = fast_exp2(om - ms);
        m = mm;
        l = l * wa + ol * wb;
#pragma unroll
        for (int i = 0; i < D / 32; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[i][r] = o[i][r] * wa + get(16 * i + r) * wb;
    }
};

// the final state of a query tile -> o rows and lse.  wl: a wave-private LDS region of ExtShape<D>::VREG bytes
template <int D>
__device__ __forceinline__ void ext_finish(const ExtState<D>& st, char* wl, bf16* o, float* lse, int64_t b, int64_t bh, int hd, int C, int n, int j0, int nq,
                                           int lane) {
    const float inv = st.l > 0.f ? 1.0f / st.l : 0.f;
    bf16x4 ob[D / 8];
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) ob[4 * dt + i][j] = f2bf(st.o[dt][4 * i + j] * inv);
    wave_rows_out<D>(wl, ob, o + (b * n + j0) * C + hd * D, C, nq, lane);
    if (lse && lane < nq) lse[bh * n + j0 + lane] = st.l > 0.f ? (st.m + __builtin_amdgcn_logf(st.l)) * LN2 : -INFINITY;   // v_log_f32 is log2
}

// an inactive row's part of a query tile: exact zeros and -inf (nthreads threads of one workgroup)
template <int D>
__device__ __forceinline__ void ext_inactive(bf16* o, float* lse, int64_t b, int64_t bh, int hd, int C, int n, int j0, int nq, int tid, int nthreads) {
    for (int i = tid; i < nq * (D / 8); i += nthreads) {
        const int r = i / (D / 8), c = i % (D / 8);
        *reinterpret_cast<u32x4*>(o + (b * n + j0 + r) * C + hd * D + 8 * c) = u32x4{0u, 0u, 0u, 0u};
    }
    if (lse && tid < nq) lse[bh * n + j0 + tid] = -INFINITY;
}

// grid (splits, ceil(n / 32), B H), 256 threads.  pos: every row's first new position, or (ROWS) the bound of pos_rows[b].
// splits == 1: o and lse are final.  Else part[((bh * tiles + tile) * splits + split) * PART] = the workgroup's state.
// GROUP (the shared-prefix form behind obte_attn_decode_shared, attention_shared.hip; ROWS false): the "chunk" is a group of n rows that
// share cache row b — the n queries of group b stand at rows b n + j of q as a chunk's do — every tile sees the keys [0, pos) and no
// other, nothing is masked by position, and the state always leaves as a partial (o and lse are not touched).
template <int D, bool ROWS, bool GROUP = false>
__global__ __launch_bounds__(EXT_WAVES * 64, 2) void attn_extend_kernel(const bf16* __restrict__ q, int64_t q_ld, const bf16* __restrict__ cache, bf16* __restrict__ o,
                                                                      float* __restrict__ lse, float* __restrict__ part, int H, int64_t T_max, int64_t v_off, int n,
                                                                      int pos, const int32_t* __restrict__ pos_rows, float qscale) {
    constexpr int NS = D / 16, ND = D / 32, NV = D / 16, CPR = D / 8;   // NV: 16-byte V pieces per lane and tile; CPR: pieces per row
    using Sh = ExtShape<D>;
    __shared__ __attribute__((aligned(16))) char smem[Sh::LDS];
    const int split = blockIdx.x, splits = gridDim.x, qt = blockIdx.y;
    const int64_t bh = blockIdx.z;
    const int64_t b = bh / H;
    const int hd = (int)(bh % H), C = H * D;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j0 = qt * EXT_QT, nq = min(n - j0, EXT_QT);
    int p = pos;
    if (ROWS) {
        p = pos_rows[b];
        if (p < 0 || p > pos) {   // (workgroup-uniform, before any barrier) with several splits the combine launch writes the zeros
            if (splits == 1) ext_inactive<D>(o, lse, b, bh, hd, C, n, j0, nq, tid, EXT_WAVES * 64);
            return;
        }
    }
    const int nk = GROUP ? p : p + j0 + nq;                      // the keys a query of this tile may see: [0, nk), nk >= 1
    const int per = ((nk + splits - 1) / splits + EXT_KT - 1) / EXT_KT * EXT_KT;
    const int k0 = min(split * per, nk), k1 = min(k0 + per, nk);
    const int qpos = p + j0 + r;                                 // this lane's query sees keys 0 .. qpos
    const int jc = min(j0 + r, n - 1);                           // (a padding query reads the chunk's last row)

    const bf16* qptr = q + (b * n + jc) * q_ld + hd * D + 8 * h;
    bf16x8 qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qptr + 16 * s);

    const bf16* kb = cache + bh * T_max * D;
    const bf16* vb = kb + v_off;
    char* vl = smem + wave * Sh::VREG;
    ExtState<D> st;
    st.clear();

    bf16x8 kf[NS];
    u32x4 vr[NV];
    // the K fragments and V pieces of the 32 keys from key0 on (key0 < k1); a key at or beyond k1 is read at k1 - 1 and its V made zero
    auto load_tile = [&](int key0) {
        const int key = key0 + r;
        const bf16* kp = kb + (int64_t)(key < k1 ? key : k1 - 1) * D + 8 * h;
#pragma unroll
        for (int s = 0; s < NS; ++s) kf[s] = *reinterpret_cast<const bf16x8*>(kp + 16 * s);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = i * 64 + lane, row = idx / CPR, ch = idx % CPR;
            const bool ok = key0 + row < k1;
            const u32x4 v = *reinterpret_cast<const u32x4*>(vb + (int64_t)(ok ? key0 + row : k1 - 1) * D + 8 * ch);
            vr[i] = ok ? v : u32x4{0u, 0u, 0u, 0u};
        }
    };
    constexpr int STEP = EXT_WAVES * EXT_KT;
    int key0 = k0 + wave * EXT_KT;
    if (key0 < k1) load_tile(key0);
    for (; key0 < k1; key0 += STEP) {
        const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        f32x16 sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[0], qf[0], zero16, 0, 0, 0);
#pragma unroll
        for (int s = 1; s < NS; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[s], qf[s], sc, 0, 0, 0);
        // V into the wave's LDS region (the region's last readers, the tile before, were issued ahead of these writes: LDS operations of
        // one wave execute in order)
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = i * 64 + lane;
            *reinterpret_cast<u32x4*>(vl + swz<D>(idx / CPR, idx % CPR)) = vr[i];
        }
        if (key0 + STEP < k1) load_tile(key0 + STEP);   // (wave-uniform) in flight under the softmax and P V below

        float mx = -INFINITY;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int key = key0 + acc_row(g, h);
            sc[g] = ((!GROUP && key > qpos) || key >= k1) ? -INFINITY : sc[g] * qscale;
            mx = fmaxf(mx, sc[g]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(st.m, mx);
        const float ms = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = fast_exp2(st.m - ms);
        st.m = m_new;
        float rs = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            sc[g] = fast_exp2(sc[g] - ms);
            rs += sc[g];
        }
        st.l = st.l * alpha + rs;
#pragma unroll
        for (int i = 0; i < ND; ++i)
#pragma unroll
            for (int g = 0; g < 16; ++g) st.o[i][g] *= alpha;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the V tile is in LDS
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const bf16x8 pf = pack8(sc, 8 * kk);
#pragma unroll
            for (int dt = 0; dt < ND; ++dt) st.o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<D>(vl, 16 * kk, dt, lane), pf, st.o[dt], 0, 0, 0);
        }
        asm volatile("" ::: "memory");
    }
    st.l += __shfl_xor(st.l, 32, 64);   // the lane pair of a query: both hold the whole normaliser from here on

    // the waves, through LDS, in wave order: [wave - 1][register][lane]
    float* mg = reinterpret_cast<float*>(smem);
    __syncthreads();   // every wave is done with its V region
    if (wave > 0) {
        float* w = mg + (wave - 1) * Sh::PART + lane;
#pragma unroll
        for (int i = 0; i < ND; ++i)
#pragma unroll
            for (int g = 0; g < 16; ++g) w[(16 * i + g) * 64] = st.o[i][g];
        w[Sh::NR * 64] = st.m;
        w[(Sh::NR + 1) * 64] = st.l;
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int wv = 1; wv < EXT_WAVES; ++wv) {
        const float* w = mg + (wv - 1) * Sh::PART + lane;
        st.merge(w[Sh::NR * 64], w[(Sh::NR + 1) * 64], [&](int g) { return w[g * 64]; });
    }
    if (!GROUP && splits == 1) {
        ext_finish<D>(st, smem + Sh::LDS - Sh::VREG, o, lse, b, bh, hd, C, n, j0, nq, lane);
        return;
    }
    float* pr = part + ((bh * gridDim.y + qt) * splits + split) * Sh::PART + lane;
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int g = 0; g < 16; ++g) pr[(16 * i + g) * 64] = st.o[i][g];
    pr[Sh::NR * 64] = st.m;
    pr[(Sh::NR + 1) * 64] = st.l;
}

// grid (ceil(n / 32), B H), one wave: lane l sums its registers of the partials in split order.  pos_rows (nullable): an inactive row
// has no partials, and gets its zeros here.
template <int D>
__global__ __launch_bounds__(64) void attn_extend_combine_kernel(const float* __restrict__ part, bf16* __restrict__ o, float* __restrict__ lse, int H, int n, int pos,
                                                                  const int32_t* __restrict__ pos_rows, int splits) {
    using Sh = ExtShape<D>;
    __shared__ __attribute__((aligned(16))) char wl[Sh::VREG];
    const int qt = blockIdx.x, lane = threadIdx.x;
    const int64_t bh = blockIdx.y;
    const int64_t b = bh / H;
    const int hd = (int)(bh % H), C = H * D;
    const int j0 = qt * EXT_QT, nq = min(n - j0, EXT_QT);
    if (pos_rows) {
        const int p = pos_rows[b];
        if (p < 0 || p > pos) {
            ext_inactive<D>(o, lse, b, bh, hd, C, n, j0, nq, lane, 64);
            return;
        }
    }
    ExtState<D> st;
    st.clear();
    const float* pr = part + (bh * gridDim.x + qt) * splits * Sh::PART + lane;
    for (int s = 0; s < splits; ++s) {
        const float* w = pr + (int64_t)s * Sh::PART;
        st.merge(w[Sh::NR * 64], w[(Sh::NR + 1) * 64], [&](int g) { return w[g * 64]; });
    }
    ext_finish<D>(st, wl, o, lse, b, bh, hd, C, n, j0, nq, lane);
}

// The rows form over the pages of a pool (obte_attn_extend_paged, include/omnibiote_hip_paged_extend.h): attn_extend_kernel<D, true, false> line for
// line — the same partition of a row's keys, the same tiles, merges and writes, so the same bits — with a kernel of its own because it takes
// three more arguments and a policy inside attn_extend_kernel moved its instantiations' instructions.  pool: K [n_pages, H, 64, hs] and V
// v_off = n_pages H 64 hs elements behind; table [B, table_ld]: entry j of row b the page of its positions [64 j, 64 j + 64), outside [0, n_pages):
// no page.  Split boundaries and wave tiles are multiples of EXT_KT = 32 keys, so a tile lies in ONE page, its index key0 / 64 is wave-uniform and
// its table entry a scalar load; the key a tile's out-of-range keys are redirected to, k1 - 1, lies in the same tile, hence in the same page.  A
// tile whose entry is no page is read from page 0, its V arrives as a selected zero and its scores are selected to -inf (attn_decode_paged_kernel's
// convention).  The entry of the wave's NEXT tile is fetched inside the load of the current one — one tile ahead, as attention_decode.hip reads
// its rounds' — so an address never waits for the table and no table load stands between two tiles' vector loads.
constexpr int PAGE = OBTE_KV_PAGE;
static_assert(PAGE % EXT_KT == 0, "a wave tile lies in one page");
template <int D>
__global__ __launch_bounds__(EXT_WAVES * 64, 2) void attn_extend_paged_kernel(const bf16* __restrict__ q, int64_t q_ld, const bf16* __restrict__ pool, bf16* __restrict__ o,
                                                                            float* __restrict__ lse, float* __restrict__ part, int H, int64_t v_off, int n, int pos,
                                                                            const int32_t* __restrict__ pos_rows, float qscale, const int32_t* __restrict__ table,
                                                                            int64_t table_ld, int n_pages) {
    constexpr int NS = D / 16, ND = D / 32, NV = D / 16, CPR = D / 8;
    using Sh = ExtShape<D>;
    __shared__ __attribute__((aligned(16))) char smem[Sh::LDS];
    const int split = blockIdx.x, splits = gridDim.x, qt = blockIdx.y;
    const int64_t bh = blockIdx.z;
    const int64_t b = bh / H;
    const int hd = (int)(bh % H), C = H * D;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j0 = qt * EXT_QT, nq = min(n - j0, EXT_QT);
    const int p = pos_rows[b];
    if (p < 0 || p > pos) {   // (workgroup-uniform, before any barrier) with several splits the combine launch writes the zeros
        if (splits == 1) ext_inactive<D>(o, lse, b, bh, hd, C, n, j0, nq, tid, EXT_WAVES * 64);
        return;
    }
    const int nk = p + j0 + nq;                                  // <= pos + n <= 64 table_ld
    const int per = ((nk + splits - 1) / splits + EXT_KT - 1) / EXT_KT * EXT_KT;
    const int k0 = min(split * per, nk), k1 = min(k0 + per, nk);
    const int qpos = p + j0 + r;
    const int jc = min(j0 + r, n - 1);

    const bf16* qptr = q + (b * n + jc) * q_ld + hd * D + 8 * h;
    bf16x8 qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qptr + 16 * s);

    const bf16* kb = pool + (int64_t)hd * PAGE * D;              // head hd's block of page 0; a page is H 64 D elements further
    const bf16* vb = kb + v_off;
    const int64_t page_stride = (int64_t)H * PAGE * D;
    const int32_t* row_table = table + b * table_ld;
    const int last_page = (k1 - 1) / PAGE;                       // (of this split; an index beyond it is clamped to it: < table_ld)
    char* vl = smem + wave * Sh::VREG;
    ExtState<D> st;
    st.clear();

    bf16x8 kf[NS];
    u32x4 vr[NV];
    constexpr int STEP = EXT_WAVES * EXT_KT;
    int ent = 0;                   // the table entry of the tile load_tile takes next (wave-uniform, as the two flags are)
    bool there_ld = false;         // the tile in kf / vr has a page
    auto load_tile = [&](int key0) {
        const int key = key0 + r;
        there_ld = (uint32_t)ent < (uint32_t)n_pages;
        // what leads from a key's number to its slot in the tile's page (page 0 where there is none)
        const int64_t t0 = (int64_t)(there_ld ? ent : 0) * page_stride - (int64_t)(key0 / PAGE * PAGE) * D;
        ent = row_table[min((key0 + STEP) / PAGE, last_page)];
        const bf16* kp = kb + t0 + (int64_t)(key < k1 ? key : k1 - 1) * D + 8 * h;
#pragma unroll
        for (int s = 0; s < NS; ++s) kf[s] = *reinterpret_cast<const bf16x8*>(kp + 16 * s);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = i * 64 + lane, row = idx / CPR, ch = idx % CPR;
            const bool ok = key0 + row < k1;
            const u32x4 v = *reinterpret_cast<const u32x4*>(vb + t0 + (int64_t)(ok ? key0 + row : k1 - 1) * D + 8 * ch);
            vr[i] = (ok && there_ld) ? v : u32x4{0u, 0u, 0u, 0u};
        }
    };
    int key0 = k0 + wave * EXT_KT;
    if (key0 < k1) {
        ent = row_table[key0 / PAGE];
        load_tile(key0);
    }
    for (; key0 < k1; key0 += STEP) {
        const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        f32x16 sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[0], qf[0], zero16, 0, 0, 0);
#pragma unroll
        for (int s = 1; s < NS; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[s], qf[s], sc, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = i * 64 + lane;
            *reinterpret_cast<u32x4*>(vl + swz<D>(idx / CPR, idx % CPR)) = vr[i];
        }
        const bool there = there_ld;                    // (of the tile whose scores stand in sc)
        if (key0 + STEP < k1) load_tile(key0 + STEP);   // (wave-uniform) in flight under the softmax and P V below

        float mx = -INFINITY;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int key = key0 + acc_row(g, h);
            sc[g] = (key > qpos || key >= k1 || !there) ? -INFINITY : sc[g] * qscale;
            mx = fmaxf(mx, sc[g]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(st.m, mx);
        const float ms = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = fast_exp2(st.m - ms);
        st.m = m_new;
        float rs = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            sc[g] = fast_exp2(sc[g] - ms);
            rs += sc[g];
        }
        st.l = st.l * alpha + rs;
#pragma unroll
        for (int i = 0; i < ND; ++i)
#pragma unroll
            for (int g = 0; g < 16; ++g) st.o[i][g] *= alpha;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the V tile is in LDS
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const bf16x8 pf = pack8(sc, 8 * kk);
#pragma unroll
            for (int dt = 0; dt < ND; ++dt) st.o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<D>(vl, 16 * kk, dt, lane), pf, st.o[dt], 0, 0, 0);
        }
        asm volatile("" ::: "memory");
    }
    st.l += __shfl_xor(st.l, 32, 64);

    float* mg = reinterpret_cast<float*>(smem);
    __syncthreads();   // every wave is done with its V region
    if (wave > 0) {
        float* w = mg + (wave - 1) * Sh::PART + lane;
#pragma unroll
        for (int i = 0; i < ND; ++i)
#pragma unroll
            for (int g = 0; g < 16; ++g) w[(16 * i + g) * 64] = st.o[i][g];
        w[Sh::NR * 64] = st.m;
        w[(Sh::NR + 1) * 64] = st.l;
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int wv = 1; wv < EXT_WAVES; ++wv) {
        const float* w = mg + (wv - 1) * Sh::PART + lane;
        st.merge(w[Sh::NR * 64], w[(Sh::NR + 1) * 64], [&](int g) { return w[g * 64]; });
    }
    if (splits == 1) {
        ext_finish<D>(st, smem + Sh::LDS - Sh::VREG, o, lse, b, bh, hd, C, n, j0, nq, lane);
        return;
    }
    float* pr = part + ((bh * gridDim.y + qt) * splits + split) * Sh::PART + lane;
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int g = 0; g < 16; ++g) pr[(16 * i + g) * 64] = st.o[i][g];
    pr[Sh::NR * 64] = st.m;
    pr[(Sh::NR + 1) * 64] = st.l;
}

bool shape_ok(int64_t B, int32_t n_head, int32_t head_dim, int64_t n_new) {
    return B > 0 && n_new > 0 && n_new < (1ll << 20) && n_head > 0 && n_head <= 1024 && (head_dim == 64 || head_dim == 128) && B * n_head <= 65535 &&
           B * n_new < (1ll << 31);
}
int64_t tiles_of(int64_t n_new) { return cdiv64(n_new, EXT_QT); }
int64_t part_floats(int32_t head_dim) { return head_dim == 128 ? ExtShape<128>::PART : ExtShape<64>::PART; }

// The default split count: decode's rule (a split is worth its workgroup and the combine launch only with EXT_MIN_KEYS keys of its own,
// more than one workgroup per CU buys nothing) on the workgroups of every query tile, and at most EXT_TILE_SPLITS / tiles of them: the
// partials of a (b, h) stay within EXT_TILE_SPLITS tiles however long the chunk is.
constexpr int64_t EXT_TARGET_WGS = 256;
constexpr int64_t EXT_MIN_KEYS = 512;
constexpr int64_t EXT_TILE_SPLITS = 16;
int64_t splits_bound(int64_t B, int32_t n_head, int64_t n_new) {
    const int64_t tiles = tiles_of(n_new);
    int64_t n = cdiv64(EXT_TARGET_WGS, B * n_head * tiles);
    if (n > EXT_TILE_SPLITS / tiles) n = EXT_TILE_SPLITS / tiles;
    if (n > OBTE_ATTN_EXTEND_MAX_SPLITS) n = OBTE_ATTN_EXTEND_MAX_SPLITS;
    return n < 1 ? 1 : n;
}

}  // namespace

extern "C" int obte_attn_extend_splits(int64_t B, int32_t n_head, int32_t head_dim, int64_t n_new, int64_t n_keys) {
    if (!shape_ok(B, n_head, head_dim, n_new) || n_keys < 1) return 1;
    const int64_t by_keys = n_keys / EXT_MIN_KEYS, bound = splits_bound(B, n_head, n_new);
    const int64_t n = by_keys < bound ? by_keys : bound;
    return n < 1 ? 1 : (int)n;
}

extern "C" int64_t obte_attn_extend_ws_bytes(int64_t B, int32_t n_head, int32_t head_dim, int64_t n_new, int32_t splits) {
    if (!shape_ok(B, n_head, head_dim, n_new) || splits < 0 || splits > OBTE_ATTN_EXTEND_MAX_SPLITS) return 0;
    const int64_t sp = splits > 0 ? splits : splits_bound(B, n_head, n_new);
    return B * n_head * tiles_of(n_new) * sp * part_floats(head_dim) * 4;
}

template <int D>
static void launch_extend(const dim3& grid, hipStream_t st, const bf16* q, int64_t q_ld, const bf16* cache, bf16* o, float* lse, float* ws, int H, int64_t T_max,
                          int64_t v_off, int n, int pos, const int32_t* pos_rows, float qscale) {
    if (pos_rows) hipLaunchKernelGGL((attn_extend_kernel<D, true>), grid, dim3(EXT_WAVES * 64), 0, st, q, q_ld, cache, o, lse, ws, H, T_max, v_off, n, pos, pos_rows, qscale);
    else hipLaunchKernelGGL((attn_extend_kernel<D, false>), grid, dim3(EXT_WAVES * 64), 0, st, q, q_ld, cache, o, lse, ws, H, T_max, v_off, n, pos, pos_rows, qscale);
    if (grid.x > 1)
        hipLaunchKernelGGL(attn_extend_combine_kernel<D>, dim3(grid.y, grid.z), dim3(64), 0, st, (const float*)ws, o, lse, H, n, pos, pos_rows, (int)grid.x);
}

// The group form's launch (attention_shared.hip has checked every argument): P cache rows of n_prefix keys, G queries each at rows
// p G + j of q, `splits` partials per (p, h, 32-query tile) to part in this file's layout.  One launch, nothing else.
void obte_attn_extend_group_partials(int head_dim, int64_t P, int G, int H, int splits, const bf16* q, int64_t q_ld, const bf16* cache, int64_t T_pre, int n_prefix,
                                     float qscale, float* part, hipStream_t st) {
    static_assert(ExtShape<64>::PART == (64 / 2 + 2) * 64 && ExtShape<128>::PART == (128 / 2 + 2) * 64, "obte_ext_part_floats (common.h) states this layout");
    const dim3 grid((unsigned)splits, (unsigned)tiles_of(G), (unsigned)(P * H));
    const int64_t v_off = P * H * T_pre * head_dim;
    if (head_dim == 128)
        hipLaunchKernelGGL((attn_extend_kernel<128, false, true>), grid, dim3(EXT_WAVES * 64), 0, st, q, q_ld, cache, nullptr, nullptr, part, H, T_pre, v_off, G, n_prefix, nullptr, qscale);
    else
        hipLaunchKernelGGL((attn_extend_kernel<64, false, true>), grid, dim3(EXT_WAVES * 64), 0, st, q, q_ld, cache, nullptr, nullptr, part, H, T_pre, v_off, G, n_prefix, nullptr, qscale);
}

extern "C" int obte_attn_extend(const obte_bf16* q, int64_t q_ld, const obte_bf16* cache, obte_bf16* o, float* lse, int64_t B, int64_t T_max, int64_t n_new,
                                int64_t pos, const int32_t* pos_rows, int32_t n_head, int32_t head_dim, float scale, int32_t splits, void* ws, int64_t ws_bytes,
                                obte_stream s) {
    OBTE_REQUIRE(q && cache && o, "obte_attn_extend: null pointer");
    OBTE_REQUIRE(n_new >= 1, "obte_attn_extend: n_new = %lld, at least one new position per row", (long long)n_new);
    OBTE_REQUIRE(shape_ok(B, n_head, head_dim, n_new) && T_max > 0 && T_max < (1ll << 24),
                 "obte_attn_extend: bad shape (head_dim 64 or 128, B * n_head <= 65535)");
    OBTE_REQUIRE(pos >= 0 && pos + n_new <= T_max, "obte_attn_extend: positions [%lld, %lld) do not fit the cache's [0, %lld)", (long long)pos,
                 (long long)(pos + n_new), (long long)T_max);
    OBTE_REQUIRE(q_ld >= (int64_t)n_head * head_dim && q_ld % 8 == 0, "obte_attn_extend: q_ld must be a multiple of 8 and at least n_head * head_dim");
    OBTE_REQUIRE((((uintptr_t)q | (uintptr_t)cache | (uintptr_t)o) & 15) == 0 && ((uintptr_t)pos_rows & 3) == 0 && ((uintptr_t)lse & 3) == 0,
                 "obte_attn_extend: q, cache and o must be 16-byte aligned, pos_rows and lse 4-byte aligned");
    OBTE_REQUIRE(splits >= 0 && splits <= OBTE_ATTN_EXTEND_MAX_SPLITS, "obte_attn_extend: splits = %d outside [0, %d]", splits, OBTE_ATTN_EXTEND_MAX_SPLITS);
    if (splits == 0) splits = obte_attn_extend_splits(B, n_head, head_dim, n_new, pos + n_new);
    if (splits > 1) {
        const int64_t need = obte_attn_extend_ws_bytes(B, n_head, head_dim, n_new, splits);
        OBTE_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0, "obte_attn_extend: %d splits need a 16-byte aligned workspace of %lld bytes, got %lld",
                     splits, (long long)need, (long long)(ws ? ws_bytes : 0));
    }
    const hipStream_t st = (hipStream_t)s;
    const int64_t BH = B * n_head;
    const float qscale = scale * LOG2E;
    const int64_t v_off = BH * T_max * head_dim;
    const int prof = obte_prof_begin(st, 104, BH, pos + n_new, head_dim);   // cache bytes read <= 4 * BH * (pos + n_new) * head_dim per query tile
    const dim3 grid((unsigned)splits, (unsigned)tiles_of(n_new), (unsigned)BH);
    if (head_dim == 128)
        launch_extend<128>(grid, st, (const bf16*)q, q_ld, (const bf16*)cache, (bf16*)o, lse, (float*)ws, n_head, T_max, v_off, (int)n_new, (int)pos, pos_rows, qscale);
    else
        launch_extend<64>(grid, st, (const bf16*)q, q_ld, (const bf16*)cache, (bf16*)o, lse, (float*)ws, n_head, T_max, v_off, (int)n_new, (int)pos, pos_rows, qscale);
    obte_prof_end(prof, st);
    OBTE_CHECK_LAUNCH("obte_attn_extend");
    return OBTE_OK;
}

// ---- the rows form over the pages of a pool (include/omnibiote_hip_paged_extend.h) ---------------------------------------------------------------
// obte_attn_extend's checks with the table in the cache's place, its split rule, its workspace and its combine launch
extern "C" int obte_attn_extend_paged(const obte_bf16* q, int64_t q_ld, const obte_bf16* pool, int64_t n_pages, const int32_t* table, int64_t table_ld, obte_bf16* o,
                                      float* lse, int64_t B, int64_t n_new, int64_t pos, const int32_t* pos_rows, int32_t n_head, int32_t head_dim, float scale,
                                      int32_t splits, void* ws, int64_t ws_bytes, obte_stream s) {
    OBTE_REQUIRE(q && pool && table && o && pos_rows, "obte_attn_extend_paged: null pointer");
    OBTE_REQUIRE(n_new >= 1, "obte_attn_extend_paged: n_new = %lld, at least one new position per row", (long long)n_new);
    OBTE_REQUIRE(shape_ok(B, n_head, head_dim, n_new) && n_pages > 0 && n_pages < (1ll << 24) && table_ld > 0 && table_ld < (1ll << 18),
                 "obte_attn_extend_paged: bad shape (head_dim 64 or 128, B * n_head <= 65535, n_pages in [1, 2^24), table_ld at least 1)");
    OBTE_REQUIRE(pos >= 0 && pos + n_new <= PAGE * table_ld, "obte_attn_extend_paged: positions [%lld, %lld) do not fit the table's [0, 64 * table_ld = %lld)",
                 (long long)pos, (long long)(pos + n_new), (long long)(PAGE * table_ld));
    OBTE_REQUIRE(q_ld >= (int64_t)n_head * head_dim && q_ld % 8 == 0, "obte_attn_extend_paged: q_ld must be a multiple of 8 and at least n_head * head_dim");
    OBTE_REQUIRE((((uintptr_t)q | (uintptr_t)pool | (uintptr_t)o) & 15) == 0 && (((uintptr_t)pos_rows | (uintptr_t)table | (uintptr_t)lse) & 3) == 0,
                 "obte_attn_extend_paged: q, pool and o must be 16-byte aligned, pos_rows, table and lse 4-byte aligned");
    OBTE_REQUIRE(splits >= 0 && splits <= OBTE_ATTN_EXTEND_MAX_SPLITS, "obte_attn_extend_paged: splits = %d outside [0, %d]", splits, OBTE_ATTN_EXTEND_MAX_SPLITS);
    if (splits == 0) splits = obte_attn_extend_splits(B, n_head, head_dim, n_new, pos + n_new);
    if (splits > 1) {
        const int64_t need = obte_attn_extend_ws_bytes(B, n_head, head_dim, n_new, splits);
        OBTE_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0,
                     "obte_attn_extend_paged: %d splits need a 16-byte aligned workspace of %lld bytes, got %lld", splits, (long long)need, (long long)(ws ? ws_bytes : 0));
    }
    const hipStream_t st = (hipStream_t)s;
    const int64_t BH = B * n_head;
    const float qscale = scale * LOG2E;
    const int64_t v_off = n_pages * n_head * PAGE * head_dim;
    const int prof = obte_prof_begin(st, 120, BH, pos + n_new, head_dim);   // (obte_attn_extend's 104 with the keys in pages)
    const dim3 grid((unsigned)splits, (unsigned)tiles_of(n_new), (unsigned)BH);
    if (head_dim == 128)
        hipLaunchKernelGGL(attn_extend_paged_kernel<128>, grid, dim3(EXT_WAVES * 64), 0, st, (const bf16*)q, q_ld, (const bf16*)pool, (bf16*)o, lse, (float*)ws, n_head,
                           v_off, (int)n_new, (int)pos, pos_rows, qscale, table, table_ld, (int)n_pages);
    else
        hipLaunchKernelGGL(attn_extend_paged_kernel<64>, grid, dim3(EXT_WAVES * 64), 0, st, (const bf16*)q, q_ld, (const bf16*)pool, (bf16*)o, lse, (float*)ws, n_head,
                           v_off, (int)n_new, (int)pos, pos_rows, qscale, table, table_ld, (int)n_pages);
    if (splits > 1) {
        if (head_dim == 128)
            hipLaunchKernelGGL(attn_extend_combine_kernel<128>, dim3(grid.y, grid.z), dim3(64), 0, st, (const float*)ws, (bf16*)o, lse, n_head, (int)n_new, (int)pos, pos_rows, (int)splits);
        else
            hipLaunchKernelGGL(attn_extend_combine_kernel<64>, dim3(grid.y, grid.z), dim3(64), 0, st, (const float*)ws, (bf16*)o, lse, n_head, (int)n_new, (int)pos, pos_rows, (int)splits);
    }
    obte_prof_end(prof, st);
    OBTE_CHECK_LAUNCH("obte_attn_extend_paged");
    return OBTE_OK;
}
