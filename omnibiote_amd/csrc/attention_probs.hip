// Attention maps (include/omnibiote_hip_probs.h): P = softmax(q k^T * scale + mask) of one layer as a tensor, the weights the fused
// forward (attention.hip) never materialises.  Two launches of one tile body, no atomics:
//   1. statistics: every 128-query block walks the key tiles of its union range and leaves (m, l) per (b, h, query) in the workspace —
//      m the row maximum in log2 units, l = sum exp2(s - m), as a pair: folded into one fp32 log-sum-exp, a row whose keys all carry
//      -1e9 would lose log l beside m;
//   2. weights: recomputes every score tile and stores exp2(s - m) / l (per head, or the heads' mean summed inside the workgroup).
// Tile body: a wave owns 32 queries, a step is one 64-key tile of one head staged in LDS by LDS-DMA (attn_common.h: the forward's image,
// ring of two).  The forward keeps the QUERY on the MFMA lane (S^T = K Q^T) because its statistics are then per lane; here the product
// is taken the other way round, S = Q K^T — the same two fragments, swapped — so that the KEY is on the lane and the 16 accumulator
// registers are 16 query rows: a store instruction then writes 32 consecutive keys of a row per lane half (whole 128-byte lines in
// fp32) straight from the registers, with no LDS transpose, and any T, aligned or not, is the same element store.  The price is paid
// in the first launch only: a lane sees a row's keys 32 apart, so it keeps a running (m, l) per register over its own keys and the 32
// lanes of a half are merged once, after the last tile (five exchanges per row, the same two products added in either partner: every
// lane ends with the same bits).  Both launches form a score with the same expression, so a weight's exponent is the difference of
// two values of one rounding history.
#include "attn_common.h"
#include "../../include/omnibiote_hip_probs.h"

namespace {
using namespace obte_attn;

constexpr int PW = 4;             // waves per workgroup
constexpr int QB = 32 * PW;       // queries per workgroup
enum { MASK_GATED = 3 };          // dense mask + key_ranges + ranges_exact: the device flag picks the range or the dense body
enum { PASS_STATS = 0, PASS_HEADS = 1, PASS_MEAN = 2 };
constexpr int MEAN_TILES = 2;     // key tiles per workgroup of the head-mean launch

struct ProbsParams {
    const bf16* qkv;
    const int32_t* key_ranges; const bf16* mask; int64_t mask_sb, mask_sh, mask_sq;
    const int32_t* gate;
    int64_t B, T; int H; float scale;
    float2* stats;                // [B][H][T]: (m in log2 units, l)
    void* out; int64_t out_sb; int out_bf16;
};

// one 32-query x 64-key tile of weights (or zeros) leaves the wave: register r of lane half h is query row acc_row(r, h), the lane's
// column is key key0 + 32 mt + (lane & 31)
template <typename OutT>
__device__ __forceinline__ void store_tile(OutT* out, int64_t row_base, int q0, int key0, int T, const f32x16 (&v)[2], float mul, int lane) {
    const int h = lane >> 5, col = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int q = q0 + acc_row(r, h);
        if (q < T) {
            OutT* row = out + row_base + (int64_t)q * T;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int key = key0 + 32 * mt + col;
                if (key < T) {
                    const float x = v[mt][r] * mul;
                    if constexpr (std::is_same<OutT, float>::value) row[key] = x; else row[key] = f2bf(x);
                }
            }
        }
    }
}

template <int D, int MODE, int PASS>
__device__ __forceinline__ void probs_body(const ProbsParams& p, char* smem) {
    constexpr int TB = 64 * 2 * D;   // bytes of one 64-key tile
    constexpr int NS = D / 16;       // k-steps over the head dim
    constexpr bool MEAN = PASS == PASS_MEAN;
    constexpr bool RANGED = MODE == MASK_RANGES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, col = lane & 31;
    const int T = (int)p.T, H = p.H, C = H * D;
    const int64_t ld = 3 * (int64_t)C;
    // per head: one workgroup per (query block, head, batch element), every key tile.  MEAN: the heads are walked inside the workgroup,
    // which would leave B * T / 128 workgroups (64 at 8 x 1024, a quarter of the CUs) — so the key tiles are divided instead, MEAN_TILES
    // per workgroup: the second launch carries nothing from one key tile to the next
    const int n_tiles = (T + 63) / 64;
    const int n_chunks = MEAN ? (n_tiles + MEAN_TILES - 1) / MEAN_TILES : 1;
    const BlockId bid = block_id(((T + QB - 1) / QB) * n_chunks, MEAN ? 1 : H);
    const int chunk = __builtin_amdgcn_readfirstlane(bid.blk % n_chunks);
    const int own_lo = MEAN ? chunk * MEAN_TILES : 0, own_hi = MEAN ? min(own_lo + MEAN_TILES, n_tiles) : n_tiles;   // the key tiles this workgroup writes
    // (block_id divides, which leaves the scalar unit; the DMA descriptor below is a scalar operand of an asm statement, where hipcc
    // cannot put the value back by itself)
    const int64_t b = __builtin_amdgcn_readfirstlane((int)bid.b);
    const int hd = __builtin_amdgcn_readfirstlane(bid.hd);
    const int q0 = __builtin_amdgcn_readfirstlane(bid.blk / n_chunks) * QB + wave * 32;   // the wave's first query (a wave past T keeps staging tiles and stores nothing)
    const float scale2 = p.scale * LOG2E;

    // key ranges first: the tile range, and with it the first LDS-DMA, depends on them
    int ks[16], ke[16];
    int lo = 0, hi = T;
    if (RANGED || (MODE == MASK_DENSE && p.key_ranges)) {
        lo = T; hi = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = b * T + min(q0 + acc_row(r, h), T - 1);
            const int a = max(p.key_ranges[row * 2], 0), e = min(p.key_ranges[row * 2 + 1], T);
            ks[r] = a; ke[r] = e;
            lo = min(lo, a); hi = max(hi, e);
        }
        block_minmax<PW>(lo, hi, reinterpret_cast<int*>(smem + 2 * TB), wave, lane);
    }
    // the union range's tiles, cut to the workgroup's own
    const int t_begin = min(max(lo / 64, own_lo), own_hi);
    const int t_end = hi > lo ? max(min((hi + 63) / 64, own_hi), t_begin) : t_begin;

    // the query fragments of head hh: the A operand, query q0 + (lane & 31) on the MFMA row
    bf16x8 qf[NS];
    auto load_q = [&](int hh) {
        const bf16* qp = p.qkv + (b * T + min(q0 + col, T - 1)) * ld + hh * D;
#pragma unroll
        for (int s = 0; s < NS; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qp + 16 * s + 8 * h);
    };
    // the statistics of the 16 rows this lane holds: first launch running values over the lane's own keys, second launch the row's pair
    float m[16], l[16];
    auto load_stats = [&](int hh) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float2 st = p.stats[(b * H + hh) * T + min(q0 + acc_row(r, h), T - 1)];
            m[r] = st.x == -INFINITY ? 0.f : st.x;
            l[r] = st.y > 0.f ? 1.0f / st.y : 0.f;   // an empty row: every weight 0
        }
    };
    if (PASS == PASS_STATS) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { m[r] = -INFINITY; l[r] = 0.f; }
    }
    if (!MEAN) load_q(hd);
    if (PASS == PASS_HEADS) load_stats(hd);

    const int nh = MEAN ? H : 1;
    const int n_steps = (t_end - t_begin) * nh;   // a step: one key tile of one head; MEAN walks the heads of a tile before the next tile
    TileDma<D, 64, PW> dma;
    dma.init(wave, lane, ld);
    auto issue = [&](int i, int t_, int hh_) {
        // (uniform, and hipcc must know it: the descriptor and the LDS address are scalar operands of the asm issue, while the
        // loop-carried counters also feed per-lane addresses)
        const int t = __builtin_amdgcn_readfirstlane(t_), hh = __builtin_amdgcn_readfirstlane(hh_);
        const int64_t row0 = (int64_t)t * 64;
        const int64_t koff = C + hh * D;
        dma.issue(p.qkv + b * T * ld + koff + row0 * ld, (((int64_t)T - row0) * ld - koff) * 2, smem + (i & 1) * TB, wave);   // rows past T arrive as zeros
    };
    if (n_steps > 0) issue(0, t_begin, MEAN ? 0 : hd);
    prologue_wait_all();
    __syncthreads();

    const int64_t out_base = b * p.out_sb + (MEAN ? 0 : (int64_t)hd * T * T);
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto store = [&](int t, const f32x16 (&v)[2], float mul) {
        if (p.out_bf16) store_tile(reinterpret_cast<bf16*>(p.out), out_base, q0, t * 64, T, v, mul, lane);
        else store_tile(reinterpret_cast<float*>(p.out), out_base, q0, t * 64, T, v, mul, lane);
    };
    if (PASS != PASS_STATS) {   // key tiles outside the block's union range: zeros, nothing computed
        const f32x16 z2[2] = {zero16, zero16};
        for (int t = own_lo; t < own_hi; ++t)
            if (t < t_begin || t >= t_end) store(t, z2, 1.0f);
    }

    f32x16 acc[2] = {zero16, zero16};   // MEAN: sum over the heads of this key tile
    const float inv_h = 1.0f / (float)H;
    int t = t_begin, hh = MEAN ? 0 : hd;   // (counted, not divided out of i: an integer division leaves the scalar unit)
    for (int i = 0; i < n_steps; ++i) {
        const bool last_head = !MEAN || hh == nh - 1;
        const int t_next = last_head ? t + 1 : t, hh_next = MEAN ? (last_head ? 0 : hh + 1) : hd;
        if (i + 1 < n_steps) issue(i + 1, t_next, hh_next);   // into the slot of step i - 1: every wave is past the barrier that ended it
        const char* Kt = smem + (i & 1) * TB;
        const int key0 = t * 64;
        if (MEAN) { load_q(hh); load_stats(hh); }

        // S = Q K^T: queries on the MFMA row (registers), keys on the column (lane)
        f32x16 sc[2];
        {
            const bf16x8 k0 = row_frag<D>(Kt, 0, 0, lane), k1 = row_frag<D>(Kt, 32, 0, lane);
            sc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[0], k0, zero16, 0, 0, 0);
            sc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[0], k1, zero16, 0, 0, 0);
        }
#pragma unroll
        for (int s = 1; s < NS; ++s) {
            const bf16x8 k0 = row_frag<D>(Kt, 0, s, lane), k1 = row_frag<D>(Kt, 32, s, lane);
            sc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[s], k0, sc[0], 0, 0, 0);
            sc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[s], k1, sc[1], 0, 0, 0);
        }
        // scores in log2 units, -inf where the key is excluded (or past T)
        const bf16* mb = MODE == MASK_DENSE ? p.mask + b * p.mask_sb + hh * p.mask_sh : nullptr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bf16* mrow = MODE == MASK_DENSE ? mb + (int64_t)min(q0 + acc_row(r, h), T - 1) * p.mask_sq : nullptr;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int key = key0 + 32 * mt + col;
                bool in = key < T;
                float v;
                if (MODE == MASK_DENSE) {
                    const float mk = in ? bf2f(mrow[key]) * LOG2E : 0.f;
                    v = __builtin_fmaf(sc[mt][r], scale2, mk);
                } else {
                    v = sc[mt][r] * scale2;
                    if (RANGED) in = key >= ks[r] && key < ke[r];
                }
                sc[mt][r] = in ? v : -INFINITY;
            }
        }
        if (PASS == PASS_STATS) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float m_new = fmaxf(m[r], fmaxf(sc[0][r], sc[1][r]));
                const float m_safe = m_new == -INFINITY ? 0.f : m_new;
                l[r] = l[r] * fast_exp2(m[r] - m_safe) + (fast_exp2(sc[0][r] - m_safe) + fast_exp2(sc[1][r] - m_safe));
                m[r] = m_new;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const float w = sc[mt][r] == -INFINITY ? 0.f : fast_exp2(sc[mt][r] - m[r]) * l[r];
                    if (MEAN) acc[mt][r] += w; else sc[mt][r] = w;
                }
        }
        dma_wait_all();   // step i + 1 has landed (and the stores of step i - 1 are out)
        __syncthreads();
        // the stores go out behind the barrier: they drain under the next step's staging and products
        if (PASS == PASS_HEADS) store(t, sc, 1.0f);
        if (MEAN && last_head) {
            store(t, acc, inv_h);
            acc[0] = zero16; acc[1] = zero16;
        }
        t = t_next; hh = hh_next;
    }

    if (PASS == PASS_STATS) {
        // a row's 32 lanes (one half of the wave) hold partial pairs: butterfly over lane bits 0..4
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) {
                const float m_o = __shfl_xor(m[r], o, 64), l_o = __shfl_xor(l[r], o, 64);
                const float m_new = fmaxf(m[r], m_o);
                const float m_safe = m_new == -INFINITY ? 0.f : m_new;
                l[r] = l[r] * fast_exp2(m[r] - m_safe) + l_o * fast_exp2(m_o - m_safe);
                m[r] = m_new;
            }
            const int q = q0 + acc_row(r, h);
            if (col == r && q < T) p.stats[(b * H + hd) * T + q] = make_float2(m[r], l[r]);
        }
    }
}

template <int D, int MODE, int PASS>
__global__ __launch_bounds__(PW * 64) void attn_probs_kernel(ProbsParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if constexpr (MODE == MASK_GATED) {
        if (__builtin_amdgcn_readfirstlane(*p.gate) == 1) probs_body<D, MASK_RANGES, PASS>(p, smem);
        else probs_body<D, MASK_DENSE, PASS>(p, smem);
    } else {
        probs_body<D, MODE, PASS>(p, smem);
    }
}

template <int D, int MODE>
int launch_probs(const ProbsParams& p, int head_mean, hipStream_t st) {
    const int smem = 2 * 64 * 2 * D + 64;   // two key tiles + block_minmax's scratch
    const int64_t nblk = cdiv64(p.T, QB);
    const dim3 block(PW * 64), grid_h((unsigned)(nblk * p.H * p.B)), grid_m((unsigned)(nblk * cdiv64(cdiv64(p.T, 64), MEAN_TILES) * p.B));
    hipLaunchKernelGGL((attn_probs_kernel<D, MODE, PASS_STATS>), grid_h, block, smem, st, p);
    OBTE_CHECK_LAUNCH("obte_attn_probs(statistics)");
    if (head_mean) hipLaunchKernelGGL((attn_probs_kernel<D, MODE, PASS_MEAN>), grid_m, block, smem, st, p);
    else hipLaunchKernelGGL((attn_probs_kernel<D, MODE, PASS_HEADS>), grid_h, block, smem, st, p);
    OBTE_CHECK_LAUNCH("obte_attn_probs(weights)");
    return OBTE_OK;
}

template <int D>
int launch_probs_mode(const ProbsParams& p, int mode, int head_mean, hipStream_t st) {
    switch (mode) {
        case MASK_NONE: return launch_probs<D, MASK_NONE>(p, head_mean, st);
        case MASK_RANGES: return launch_probs<D, MASK_RANGES>(p, head_mean, st);
        case MASK_DENSE: return launch_probs<D, MASK_DENSE>(p, head_mean, st);
        default: return launch_probs<D, MASK_GATED>(p, head_mean, st);
    }
}
}  // namespace

extern "C" int64_t obte_attn_probs_args_bytes(void) { return (int64_t)sizeof(obte_attn_probs_args); }

extern "C" int64_t obte_attn_probs_ws_bytes(int64_t B, int64_t T, int32_t n_head) {
    if (B < 1 || T < 1 || n_head < 1 || B >= 65536 || n_head >= 65536 || T >= (1 << 24)) return 0;
    return B * n_head * T * (int64_t)sizeof(float2);
}

extern "C" int obte_attn_probs(const obte_attn_probs_args* a, obte_stream s) {
    const char* who = "obte_attn_probs";
    OBTE_REQUIRE(a, "%s: null args", who);
    OBTE_REQUIRE(a->qkv, "%s: null qkv", who);
    OBTE_REQUIRE(a->out, "%s: null out", who);
    OBTE_REQUIRE(a->ws, "%s: null ws", who);
    OBTE_REQUIRE(a->B > 0 && a->T > 0 && a->n_head > 0 && a->B < 65536 && a->n_head < 65536, "%s: bad B/T/H", who);
    OBTE_REQUIRE(a->head_dim == 64 || a->head_dim == 128, "%s: head_dim must be 64 or 128 (got %d)", who, (int)a->head_dim);
    OBTE_REQUIRE(a->T < (1 << 24), "%s: T too large", who);
    OBTE_REQUIRE(a->B * a->n_head * cdiv64(a->T, QB) < (1ll << 30), "%s: too many (batch, head, row block) workgroups", who);
    OBTE_REQUIRE((a->out_bf16 == 0 || a->out_bf16 == 1) && (a->head_mean == 0 || a->head_mean == 1), "%s: out_bf16 and head_mean are 0 or 1", who);
    OBTE_REQUIRE(a->out_sb >= (a->head_mean ? 1 : (int64_t)a->n_head) * a->T * a->T, "%s: out_sb is smaller than a batch element's maps", who);
    OBTE_REQUIRE(a->ws_bytes >= obte_attn_probs_ws_bytes(a->B, a->T, a->n_head), "%s: ws_bytes %lld is below obte_attn_probs_ws_bytes() = %lld", who,
                 (long long)a->ws_bytes, (long long)obte_attn_probs_ws_bytes(a->B, a->T, a->n_head));
    OBTE_REQUIRE_ALIGNED(who, a->qkv, "qkv", 16);
    OBTE_REQUIRE_ALIGNED(who, a->ws, "ws", 8);
    OBTE_REQUIRE_ALIGNED(who, a->out, "out", a->out_bf16 ? 2 : 4);
    OBTE_REQUIRE_ALIGNED(who, a->key_ranges, "key_ranges", 4);
    OBTE_REQUIRE_ALIGNED(who, a->mask, "mask", 2);
    ProbsParams p = {};
    p.qkv = (const bf16*)a->qkv;
    p.key_ranges = a->key_ranges; p.mask = (const bf16*)a->mask; p.mask_sb = a->mask_sb; p.mask_sh = a->mask_sh; p.mask_sq = a->mask_sq;
    p.B = a->B; p.T = a->T; p.H = a->n_head; p.scale = a->scale;
    p.stats = (float2*)a->ws; p.out = a->out; p.out_sb = a->out_sb; p.out_bf16 = a->out_bf16;
    int mode = a->mask ? MASK_DENSE : (a->key_ranges ? MASK_RANGES : MASK_NONE);   // a dense mask wins (attention.hip mask_mode)
    if (mode == MASK_DENSE && a->key_ranges && a->ranges_exact) { mode = MASK_GATED; p.gate = a->ranges_exact; }
    hipStream_t st = (hipStream_t)s;
    // kind 121: (maps stored = B * (1 or n_head), T, head size); bytes stored = maps * T * T * (4 or 2)
    const int prof = obte_prof_begin(st, 121, a->B * (a->head_mean ? 1 : a->n_head), a->T, a->head_dim);
    const int rc = a->head_dim == 128 ? launch_probs_mode<128>(p, mode, a->head_mean, st) : launch_probs_mode<64>(p, mode, a->head_mean, st);
    obte_prof_end(prof, st);
    return rc;
}
