// Host side of the bf16 GEMM family: argument validation, the plan table, plan resolution, kernel parameters, profiler records and
// the extern "C" GEMM entry points.  The structures themselves (gemm_bf16_v1.hip, gemm_bf16_v2.hip: 2, 3, 4 and the grouped launch,
// gemm_bf16_v7.hip) each hold their kernels and one launcher; which forms they have is gemm_has_form (gemm_common.h).
#include "gemm_common.h"
#include <string.h>
#include <map>
#include <mutex>
#include <tuple>

using namespace obte_gemm_v2;

int gemm_no_form(int s, int bn, bool ak, bool bk, int epi, bool split) {
    obte_set_error("obte_gemm_bf16: structure %d (%d wide) has no form for a_kmajor %d, b_kmajor %d, epilogue %d%s", s, bn, (int)ak, (int)bk, epi,
                   split ? ", split-K" : "");
    return OBTE_EINVAL;
}

static int validate_args(const obte_gemm_args* g) {
    OBTE_REQUIRE(g && g->a && g->b && (g->d || (g->epilogue == OBTE_EPI_ACC32 && g->acc32_mode != OBTE_ACC32_LAST)), "obte_gemm_bf16: null pointer");
    OBTE_REQUIRE_ALIGNED("obte_gemm_bf16", g->a, "a", 16);
    OBTE_REQUIRE_ALIGNED("obte_gemm_bf16", g->b, "b", 16);
    OBTE_REQUIRE_ALIGNED("obte_gemm_bf16", g->d, "d", 16);
    OBTE_REQUIRE_ALIGNED("obte_gemm_bf16", g->aux, "aux", 16);
    OBTE_REQUIRE_ALIGNED("obte_gemm_bf16", g->d2, "d2", 16);
    OBTE_REQUIRE_ALIGNED("obte_gemm_bf16", g->rope_cos, "rope_cos", 16);
    OBTE_REQUIRE_ALIGNED("obte_gemm_bf16", g->rope_sin, "rope_sin", 16);
    OBTE_REQUIRE_ALIGNED("obte_gemm_bf16", g->acc32, "acc32", 16);
    OBTE_REQUIRE(g->M > 0 && g->N > 0 && g->K > 0, "obte_gemm_bf16: empty problem M=%lld N=%lld K=%lld",
                 (long long)g->M, (long long)g->N, (long long)g->K);
    OBTE_REQUIRE(g->lda % 8 == 0 && g->ldb % 8 == 0 && g->ldd % 8 == 0 && g->N % 8 == 0,
                 "obte_gemm_bf16: lda/ldb/ldd/N must be multiples of 8 (16-byte rows)");
    OBTE_REQUIRE(!(g->a_kmajor) || g->K % 64 == 0, "obte_gemm_bf16: k-contiguous A needs K %% 64 == 0 (K=%lld)", (long long)g->K);
    OBTE_REQUIRE(!(g->b_kmajor) || g->K % 64 == 0, "obte_gemm_bf16: k-contiguous B needs K %% 64 == 0 (K=%lld)", (long long)g->K);
    OBTE_REQUIRE(g->a_kmajor ? g->lda >= g->K : g->lda >= g->M, "obte_gemm_bf16: lda too small");
    OBTE_REQUIRE(g->b_kmajor ? g->ldb >= g->K : g->ldb >= g->N, "obte_gemm_bf16: ldb too small");
    OBTE_REQUIRE(g->ldd >= g->N, "obte_gemm_bf16: ldd too small");
    OBTE_REQUIRE(g->lda <= 1 << 20 && g->ldb <= 1 << 20, "obte_gemm_bf16: leading dimension too large");
    if (g->epilogue == OBTE_EPI_ADD || g->epilogue == OBTE_EPI_GELU_BWD || g->epilogue == OBTE_EPI_ADD_DROPOUT) OBTE_REQUIRE(g->aux, "obte_gemm_bf16: epilogue needs aux");
    if (g->epilogue == OBTE_EPI_ADD_DROPOUT) OBTE_REQUIRE(g->dropout_p >= 0.f && g->dropout_p < 1.f, "obte_gemm_bf16: dropout p must be in [0,1)");
    if (g->epilogue == OBTE_EPI_ROPE_QK)
        OBTE_REQUIRE(g->rope_cos && g->rope_sin && g->rope_T > 0 && g->rope_head_dim > 0 && g->rope_head_dim % 8 == 0 && g->N % 3 == 0 &&
                         (g->N / 3) % g->rope_head_dim == 0,
                     "obte_gemm_bf16: EPI_ROPE_QK needs cos/sin tables, T, head_dim %% 8 == 0 and N = 3 * n_head * head_dim");
    if (g->epilogue == OBTE_EPI_GELU) OBTE_REQUIRE(g->d2, "obte_gemm_bf16: GELU epilogue needs d2");
    if (g->epilogue == OBTE_EPI_GELU_ACT) OBTE_REQUIRE(g->a_kmajor && g->b_kmajor, "obte_gemm_bf16: EPI_GELU_ACT exists in the x W^T layout only (a_kmajor = b_kmajor = 1)");
    if (g->epilogue == OBTE_EPI_ACC32)
        OBTE_REQUIRE(g->acc32 && g->acc32_mode >= OBTE_ACC32_FIRST && g->acc32_mode <= OBTE_ACC32_LAST && !g->a_kmajor && !g->b_kmajor && g->ldd == g->N,
                     "obte_gemm_bf16: EPI_ACC32 needs the fp32 buffer, a mode (OBTE_ACC32_*), the weight-gradient layout (a_kmajor = b_kmajor = 0) and ldd == N");
    else
        OBTE_REQUIRE(!g->acc32 && g->acc32_mode == 0, "obte_gemm_bf16: acc32 / acc32_mode belong to EPI_ACC32");
    if (g->epilogue != OBTE_EPI_NONE && g->epilogue != OBTE_EPI_ADD && g->epilogue != OBTE_EPI_ACC32)
        OBTE_REQUIRE(g->alpha == 1.0f, "obte_gemm_bf16: alpha != 1 only with EPI_NONE / EPI_ADD / EPI_ACC32");
    return OBTE_OK;
}

// ---- plans: (structure, tile width, split-K) ------------------------------------------------------------------------------------
// Structure 1: gemm_bf16_v1.hip; 2 / 3 / 4: gemm_bf16_v2.hip (K-tile ring / half-tile ring / half-tile ring at two workgroups per CU);
// 7: gemm_bf16_v7.hip (the persistent continuous-ring structure).
struct Plan { int structure; int bn; int splits; };

// Built-in heuristic (structure 2): prefer the 256-wide tile (higher FLOP per loaded byte) whenever it still yields at least one
// workgroup per CU, directly or through a split of a long K; otherwise the 128-wide tile.  Split-K needs a workspace, epilogue NONE
// or ADD and ldd == N.
static int splits_for(int64_t tiles, int64_t nk) {
    if (tiles >= 200 || nk < 16) return 1;
    int s = (int)(256 / tiles);   // the largest split whose tiles * s workgroups still fit ONE round of the 256 CUs (rounding up instead
                                  // put e.g. 20 tiles x 13 = 260 workgroups into two rounds: the readout's row-compact input gradient)
    while (s > 1 && nk / s < 8) --s;
    return s < 1 ? 1 : (s > 16 ? 16 : s);
}
static Plan make_plan(int64_t M, int64_t N, int64_t K, bool can_split) {
    const int64_t nk = cdiv64(K, BKT);
    const int64_t tm = cdiv64(M, BM);
    const int64_t t256 = tm * cdiv64(N, 256);
    const int s256 = can_split ? splits_for(t256, nk) : 1;
    const int bn = (N >= 256 && t256 * s256 >= 200) ? 256 : 128;
    const int64_t tiles = tm * cdiv64(N, bn);
    return Plan{2, bn, can_split ? splits_for(tiles, nk) : 1};
}

// The shape conditions under which a structure runs a plan as given (beside having the form: gemm_has_form), and what runs instead.
// Structure 7: whole 256 x 256 tiles, at least one per CU, eight half-steps or more per tile (the ring is refilled four half-steps ahead
// across tiles).  Structures 3 and 4: the half-tile rings need two K-tiles (four half-steps) or more in every split.
static bool runs_as_given(const Plan& pl, const obte_gemm_args* g) {
    if (!gemm_has_form(pl.structure, pl.bn, g->a_kmajor != 0, g->b_kmajor != 0, g->epilogue, pl.splits > 1)) return false;
    if (pl.structure == 7)
        return g->M % BM == 0 && g->N % 256 == 0 && g->K % BKT == 0 && g->K >= 4 * BKT && (g->M / BM) * (g->N / 256) >= 256 &&
               (g->epilogue != OBTE_EPI_ADD || g->aux != nullptr) &&
               g->ldd < (1ll << 24) &&                        // (32-bit element offsets inside a wave's 64-row tile; the tile origin is 64-bit)
               g->M * g->N * 2 <= (256ll << 20);              // (an output beyond the Infinity Cache wants non-temporal stores: structures 2 / 3)
    if (pl.structure == 3 || pl.structure == 4) {
        const int64_t nk = cdiv64(g->K, BKT), k_per_split = cdiv64(nk, pl.splits);
        return k_per_split >= 2 && nk - (pl.splits - 1) * k_per_split >= 2;
    }
    return true;
}
static bool fall_back(Plan& pl, const obte_gemm_args* g) {   // false: nothing to fall back to (the launcher reports the missing form)
    switch (pl.structure) {
        case 1: if (g->epilogue != OBTE_EPI_ACC32) return false;      // (a NONE plan borrowed for the fp32 sum, which structure 1 lacks)
                pl = make_plan(g->M, g->N, g->K, false); return true;
        case 7: pl = Plan{3, 256, 1}; return true;                    // the same main loop, one tile per workgroup
        case 3: case 4: pl.structure = 2; return true;               // the K-tile ring at the same width and split
        case 2: if (pl.bn != 192) return false;                      // the 192-wide tile: the heuristic, no split
                pl = make_plan(g->M, g->N, g->K, false); return true;
    }
    return false;
}

// Tuned plans: (layout, epilogue, M, N, K) -> plan, filled by the host-side tuner (omnibiote_amd/tune.py), which times the candidates
// on the actual device once per shape.  Lookups are per call, under a mutex.
typedef std::tuple<int, int, int64_t, int64_t, int64_t> PlanKey;
static std::mutex g_plan_mu;
static std::map<PlanKey, Plan> g_plans;
static int layout_of(const obte_gemm_args* g) { return (g->a_kmajor ? 2 : 0) + (g->b_kmajor ? 1 : 0); }

// A plan tuned for (m, n, k) serves (M, N, K) when the shapes are equal, or when exactly one dimension differs and by at most 20 %:
// the readout's row-compact backward contracts over the MLM-masked rows of a micro-batch, whose count changes from call to call
// (about 15 % of the rows), so its two shapes never match a tuned entry exactly.
static bool serves(const PlanKey& key, int64_t M, int64_t N, int64_t K) {
    auto near = [](int64_t a, int64_t b) { return a * 5 >= b * 4 && a * 5 <= b * 6; };
    const int64_t m = std::get<2>(key), n = std::get<3>(key), k = std::get<4>(key);
    const int same = (m == M) + (n == N) + (k == K);
    return same == 3 || (same == 2 && near(m, M) && near(n, N) && near(k, K));
}

static bool lookup_plan(const obte_gemm_args* g, Plan* out, bool* near_match) {
    std::lock_guard<std::mutex> lk(g_plan_mu);
    const int lay = layout_of(g);
    auto it = g_plans.find(PlanKey(lay, g->epilogue, g->M, g->N, g->K));
    if (it == g_plans.end() && (g->epilogue == OBTE_EPI_ADD || g->epilogue == OBTE_EPI_ACC32))   // accumulate-into-grad (bf16 or fp32) reuses the plan tuned for the plain form
        it = g_plans.find(PlanKey(lay, OBTE_EPI_NONE, g->M, g->N, g->K));
    if (it == g_plans.end() && g->epilogue == OBTE_EPI_ROPE_QK)       // the c_attn projection: plan of the plain form
        it = g_plans.find(PlanKey(lay, OBTE_EPI_NONE, g->M, g->N, g->K));
    if (it == g_plans.end() && g->epilogue == OBTE_EPI_ADD_DROPOUT)   // same main loop as the residual-add form
        it = g_plans.find(PlanKey(lay, OBTE_EPI_ADD, g->M, g->N, g->K));
    if (it == g_plans.end() && g->epilogue == OBTE_EPI_GELU_ACT)      // the activation alone: the main loop of the two-output form
        it = g_plans.find(PlanKey(lay, OBTE_EPI_GELU, g->M, g->N, g->K));
    if (it == g_plans.end()) {   // a near match: an entry with the same layout and epilogue (ADD: NONE's)
        const int epi = (g->epilogue == OBTE_EPI_ADD || g->epilogue == OBTE_EPI_ACC32) ? OBTE_EPI_NONE : g->epilogue;
        for (auto jt = g_plans.begin(); jt != g_plans.end(); ++jt)
            if (std::get<0>(jt->first) == lay && std::get<1>(jt->first) == epi && serves(jt->first, g->M, g->N, g->K)) {
                it = jt;
                *near_match = true;
                break;
            }
    }
    if (it == g_plans.end()) return false;
    *out = it->second;
    return true;
}

// The plan that runs g with a workspace of workspace_bytes (none: null): the tuned plan of the shape or the heuristic; a borrowed split
// count trimmed to one round; no split without a workspace that holds it; splits that would be empty dropped; then, while the plan's
// structure cannot run it as given, its fallback.
static Plan resolve(const obte_gemm_args* g, const void* workspace, int64_t workspace_bytes) {
    const bool can_split = workspace && (g->epilogue == OBTE_EPI_NONE || g->epilogue == OBTE_EPI_ADD || g->epilogue == OBTE_EPI_ACC32) && g->ldd == g->N;
    Plan pl;
    bool near_match = false;
    if (!lookup_plan(g, &pl, &near_match)) pl = make_plan(g->M, g->N, g->K, can_split);
    if (near_match && pl.splits > 1) {   // a borrowed split count must still fit one round for THIS tile count (1288 rows: 24 tiles x 12 = 288)
        const int64_t tiles = cdiv64(g->M, BM) * cdiv64(g->N, pl.bn);
        while (pl.splits > 1 && tiles <= 256 && tiles * pl.splits > 256) --pl.splits;
    }
    if (pl.splits > 1 && (!can_split || (int64_t)pl.splits * g->M * g->N * 4 > workspace_bytes)) pl = make_plan(g->M, g->N, g->K, false);
    const int64_t nk = cdiv64(g->K, BKT);
    pl.splits = (int)cdiv64(nk, cdiv64(nk, pl.splits));
    while (!runs_as_given(pl, g) && fall_back(pl, g)) {}
    return pl;
}

// Kernel parameters of g under plan pl (structures 2, 3, 4, 7 and the grouped launch; obte_gemm_v1_launch derives its own)
static void fill_params(const obte_gemm_args* g, void* workspace, const Plan& pl, GemmParams& p) {
    p.a = (const bf16*)g->a; p.b = (const bf16*)g->b; p.d = (bf16*)g->d; p.aux = (const bf16*)g->aux; p.d2 = (bf16*)g->d2;
    p.slab = (float*)workspace;
    p.M = g->M; p.N = g->N; p.K = g->K; p.lda = g->lda; p.ldb = g->ldb; p.ldd = g->ldd;
    p.a_elems = (g->a_kmajor ? g->M : g->K) * g->lda;
    p.b_elems = (g->b_kmajor ? g->N : g->K) * g->ldb;
    p.store_rows = p.M;
    p.delay_sleeps = 0;
    p.dbg_times = nullptr;
    p.nt_store = (g->M * g->N * 2 > (256ll << 20)) ? 1 : 0;
    // the GELU epilogue's d (the derivative, 67 MB at the hot-path shape) is read again only in the backward pass: stored
    // non-temporally it does not push the activation d2 — the next GEMM's operand — and the operand panels out of L2 /
    // Infinity Cache (c_fc + GELU 97.8 -> 94.5 us, cold operands)
    if (g->epilogue == OBTE_EPI_GELU) p.nt_store = 1;
    p.tiles_m = (int)cdiv64(g->M, BM); p.tiles_n = (int)cdiv64(g->N, pl.bn);
    const int64_t nk = cdiv64(g->K, BKT);
    p.k_per_split = (int)cdiv64(nk, pl.splits);
    p.splits = (int)cdiv64(nk, p.k_per_split);   // no empty splits
    p.alpha = g->alpha;
    p.rope_cos = g->rope_cos; p.rope_sin = g->rope_sin; p.rope_T = g->rope_T; p.rope_hs = g->rope_head_dim;
    p.drop = make_drop(g->epilogue == OBTE_EPI_ADD_DROPOUT ? g->dropout_p : 0.f, g->dropout_seed, (uint32_t)g->dropout_site);
    p.acc32 = g->acc32; p.acc32_mode = g->acc32_mode;
#ifdef OBTE_DEBUG_HOOKS
    {   // timing-only diagnostics of the debug build (results are wrong): zero-record descriptors drop every LDS-DMA / no stores
        static int noload = -1, nostore = -1, exit_now = -1;
        if (noload < 0) {
            const char* e = getenv("OBTE_GEMM_DEBUG");
            nostore = (e && strstr(e, "nostore")) ? 1 : 0;
            exit_now = (e && strstr(e, "exit")) ? 1 : 0;
            noload = (e && strstr(e, "noload")) ? 1 : 0;
            if (noload || nostore || exit_now) fprintf(stderr, "libomnibiote_hip (DEBUG build): OBTE_GEMM_DEBUG=%s is active — GEMM results are WRONG, timing only\n", e);
        }
        if (noload) { p.a_elems = 0; p.b_elems = 0; }
        if (exit_now) p.store_rows = -1; else if (nostore) p.store_rows = 0;
        static int delay = -1;
        if (delay < 0) { const char* d = getenv("OBTE_GEMM_V4_DELAY"); delay = d ? atoi(d) : 0; }
        p.delay_sleeps = delay;
    }
#endif
}

// Profiler record kind, as bench.py decodes it: a single launch 4 x layout + epilogue + 1000 x structure (a split-K reduce is inside the
// same record); a grouped launch (last: its last problem) 32, + 1 if its first and last problems differ in layout, + 2 if it accumulates.
static int prof_kind(const obte_gemm_args* g, int structure, const obte_gemm_args* last = nullptr) {
    if (last) return 32 + (layout_of(last) != layout_of(g) ? 1 : 0) + ((g->epilogue == OBTE_EPI_ADD || g->epilogue == OBTE_EPI_ACC32) ? 2 : 0);
    return 4 * layout_of(g) + (g->epilogue == OBTE_EPI_ACC32 ? OBTE_EPI_ADD : g->epilogue) + 1000 * structure;   // (the fp32 sum is recorded as the accumulate form it replaces)
}

// The grouped and the row-dot launches pass no dropout and no RoPE tables, whatever the descriptor holds (their epilogues read neither)
static void no_drop_no_rope(GemmParams& p) {
    p.drop = make_drop(0.f, 0, 0);
    p.rope_cos = nullptr; p.rope_sin = nullptr; p.rope_T = 0; p.rope_hs = 0;
}

static int launch_plan(const Plan& pl, const GemmParams& p, const obte_gemm_args* g, hipStream_t st) {
    const bool ak = g->a_kmajor != 0, bk = g->b_kmajor != 0;
    switch (pl.structure) {
        case 1: return obte_gemm_v1_launch(p, ak, bk, g->epilogue, st);
        case 2: return pl.bn == 256 ? obte_gemm_v2_launch<256>(p, ak, bk, g->epilogue, st)
                     : pl.bn == 192 ? obte_gemm_v2_launch<192>(p, ak, bk, g->epilogue, st)
                                    : obte_gemm_v2_launch<128>(p, ak, bk, g->epilogue, st);
        case 3: return obte_gemm_v3_launch(p, ak, bk, g->epilogue, st);
        case 4: return obte_gemm_v4_launch(p, ak, bk, g->epilogue, st);
        case 7: return obte_gemm_v7_launch(p, ak, bk, g->epilogue, st);
    }
    return gemm_no_form(pl.structure, pl.bn, ak, bk, g->epilogue, p.splits > 1);
}

#ifdef OBTE_DEBUG_HOOKS
// OBTE_GEMM_TIMES=1 (debug build): where a GEMM launch spends its time, from s_memrealtime stamps (100 MHz) of every workgroup
#include <vector>
static unsigned long long* debug_gemm_times_buffer(int64_t groups) {
    static int on = -1;
    static unsigned long long* buf = nullptr;
    static int64_t cap = 0;
    if (on < 0) { const char* e = getenv("OBTE_GEMM_TIMES"); on = (e && e[0] == '1') ? 1 : 0; }
    if (!on) return nullptr;
    if (cap < groups) {
        if (buf) (void)hipFree(buf);
        if (hipMalloc((void**)&buf, (size_t)groups * 64) != hipSuccess) { buf = nullptr; cap = 0; return nullptr; }
        cap = groups;
    }
    (void)hipMemset(buf, 0, (size_t)groups * 64);
    return buf;
}
static void debug_gemm_report(const GemmParams& p, int variant, int epi, hipStream_t st) {
    const int n = p.tiles_m * p.tiles_n * p.splits;
    static std::vector<unsigned long long> h;
    h.resize((size_t)n * 8);
    if (hipStreamSynchronize(st) != hipSuccess) return;
    if (hipMemcpy(h.data(), p.dbg_times, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    unsigned long long t0 = ~0ull, tend = 0;
    for (int i = 0; i < n; ++i) { if (h[(size_t)i * 8] && h[(size_t)i * 8] < t0) t0 = h[(size_t)i * 8]; if (h[(size_t)i * 8 + 4] > tend) tend = h[(size_t)i * 8 + 4]; }
    // workgroups of the first wave of residents (entered within 2 us of the first) and the rest (later rounds)
    double seg[2][4] = {{0}}, entry[2] = {0, 0}, done[2] = {0, 0}, ep1[2] = {0, 0}, ep2[2] = {0, 0}, ep3[2] = {0, 0}; int cnt[2] = {0, 0};
    for (int i = 0; i < n; ++i) {
        const unsigned long long* r = &h[(size_t)i * 8];
        if (!r[0]) continue;
        const int c = (r[0] - t0) > 200 ? 1 : 0;
        cnt[c]++; entry[c] += (double)(r[0] - t0); done[c] += (double)(r[4] - t0);
        for (int k = 0; k < 4; ++k) seg[c][k] += (double)(r[k + 1] - r[k]);
        if (r[5] && r[6]) { ep1[c] += (double)(r[5] - r[2]); ep2[c] += (double)(r[6] - r[5]); ep3[c] += (double)(r[7] - r[6]); }   // epilogue: until every wave is out of the loop / staging written and published
    }
    fprintf(stderr, "[gemm v%d epi %d %lldx%lldx%lld, %d workgroups, us] span %.2f", variant, epi, (long long)p.M, (long long)p.N, (long long)p.K, n, (tend - t0) * 0.01);
    for (int c = 0; c < 2; ++c)
        if (cnt[c]) fprintf(stderr, " | %s %d: entry +%.2f, prologue %.2f, loop %.2f, epilogue issue %.2f (all waves out of the loop %.2f + staging %.2f + read back %.2f + arithmetic, stores), drain %.2f, done +%.2f", c ? "later" : "first", cnt[c], entry[c] / cnt[c] * 0.01,
                            seg[c][0] / cnt[c] * 0.01, seg[c][1] / cnt[c] * 0.01, seg[c][2] / cnt[c] * 0.01, ep1[c] / cnt[c] * 0.01, ep2[c] / cnt[c] * 0.01, ep3[c] / cnt[c] * 0.01, seg[c][3] / cnt[c] * 0.01, done[c] / cnt[c] * 0.01);
    fprintf(stderr, "\n");
}
#endif

// ---- entry points ----------------------------------------------------------------------------------------------------------------
extern "C" int obte_gemm_plan_set(int a_kmajor, int b_kmajor, int epilogue, int64_t M, int64_t N, int64_t K, int variant,
                                  int bn, int splits) {
    static const char* const forms[] = {nullptr, "the first structure is 128 wide, no split-K",
                                        "the K-tile ring is 128, 192 or 256 wide, split-K with epilogue NONE, ADD or ACC32; ACC32 in the weight-gradient layout",
                                        "the four-half-stage structure is 256 wide, split-K with epilogue NONE, ADD or ACC32; ACC32 in the weight-gradient layout",
                                        "the two-workgroups-per-CU structure is 128 wide, split-K with epilogue NONE, ADD or ACC32; ACC32 in the weight-gradient layout", nullptr, nullptr,
                                        "the persistent continuous-ring structure is 256 wide, no split-K, x W^T and dy W layouts with their epilogues"};
    OBTE_REQUIRE(variant >= 1 && variant <= 7 && forms[variant] && (bn == 128 || bn == 256 || bn == 192) && splits >= 1 && splits <= 64,
                 "obte_gemm_plan_set: bad plan");
    OBTE_REQUIRE(gemm_has_form(variant, bn, a_kmajor != 0, b_kmajor != 0, epilogue, splits > 1), "obte_gemm_plan_set: %s",
                 bn == 192 && variant != 7 ? "the 192-wide tile exists for the K-tile ring, k-contiguous operands, no split-K" : forms[variant]);
    std::lock_guard<std::mutex> lk(g_plan_mu);
    g_plans[PlanKey((a_kmajor ? 2 : 0) + (b_kmajor ? 1 : 0), epilogue, M, N, K)] = Plan{variant, bn, splits};
    return OBTE_OK;
}
extern "C" int obte_gemm_plan_clear(void) {
    std::lock_guard<std::mutex> lk(g_plan_mu);
    g_plans.clear();
    return OBTE_OK;
}
// the largest split any call of this shape may take: the heuristic's, or that of any plan (every layout and epilogue) that serves it
extern "C" int64_t obte_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K) {
    int splits = make_plan(M, N, K, true).splits;
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        bool tuned = false;
        int ts = 1;
        for (auto& kv : g_plans)
            if (serves(kv.first, M, N, K)) {
                tuned = true;
                if (kv.second.splits > ts) ts = kv.second.splits;
            }
        if (tuned) splits = ts > splits ? ts : splits;
    }
    return splits > 1 ? (int64_t)splits * M * N * 4 : 0;
}

extern "C" int obte_gemm_bf16_ws(const obte_gemm_args* g, void* workspace, int64_t workspace_bytes, obte_stream s) {
    OBTE_REQUIRE_ALIGNED("obte_gemm_bf16", workspace, "workspace", 16);
    { const int vrc = validate_args(g); if (vrc != OBTE_OK) return vrc; }
    hipStream_t st = (hipStream_t)s;
    const Plan pl = resolve(g, workspace, workspace_bytes);
    OBTE_REQUIRE(pl.structure == 1 || cdiv64(g->M, BM) * cdiv64(g->N, pl.bn) < (1ll << 26), "obte_gemm_bf16: too many tiles");
    GemmParams p;
    fill_params(g, workspace, pl, p);
#ifdef OBTE_DEBUG_HOOKS
    if (pl.structure != 1) p.dbg_times = debug_gemm_times_buffer((int64_t)p.tiles_m * p.tiles_n * p.splits);
#endif
    const int prof = obte_prof_begin(st, prof_kind(g, pl.structure), g->M, g->N, g->K);
    int rc = launch_plan(pl, p, g, st);
#ifdef OBTE_DEBUG_HOOKS
    if (rc == OBTE_OK && p.dbg_times && pl.structure >= 2 && pl.structure <= 4) debug_gemm_report(p, pl.structure, g->epilogue, st);   // (7 reports itself)
#endif
    if (rc == OBTE_OK && p.splits > 1)
        rc = g->epilogue == OBTE_EPI_ACC32 ? obte_gemm_splitk_reduce_acc32(p, st) : obte_gemm_splitk_reduce(p, g->epilogue == OBTE_EPI_ADD ? p.aux : nullptr, st);
    obte_prof_end(prof, st);
    return rc;
}

extern "C" int obte_gemm_bf16(const obte_gemm_args* g, obte_stream s) { return obte_gemm_bf16_ws(g, nullptr, 0, s); }

// common.h: the plain dy W product with the row-dot epilogue, on structure 7 or not at all
extern "C" int obte_gemm_rowdot_bf16(const obte_gemm_args* g, const obte_bf16* other, float* rowdot, int64_t T, int32_t head_dim, obte_stream s) {
    { const int vrc = validate_args(g); if (vrc != OBTE_OK) return vrc; }
    OBTE_REQUIRE(other && rowdot && T > 0, "obte_gemm_rowdot_bf16: null pointer");
    OBTE_REQUIRE(g->epilogue == OBTE_EPI_NONE && g->a_kmajor && !g->b_kmajor && g->alpha == 1.0f, "obte_gemm_rowdot_bf16: the plain dy W product only");
    static const bool off = [] { const char* e = getenv("OBTE_GEMM_ROWDOT"); return e && e[0] == '0'; }();   // (A/B timing: the prep launch forms delta instead)
    const Plan pl{7, 256, 1};
    obte_gemm_args g2 = *g;
    g2.epilogue = OBTE_EPI_ROWDOT;
    if (off || head_dim != 128 || g->N % 128 != 0 || g->M % T != 0 || T >= (1ll << 31) || g->M >= (1ll << 31) || !runs_as_given(pl, &g2))
        return OBTE_ROWDOT_NOT_TAKEN;
    hipStream_t st = (hipStream_t)s;
    GemmParams p;
    fill_params(g, nullptr, pl, p);
    p.aux = (const bf16*)other;
    p.slab = rowdot;                      // (no split-K here: the slot carries the row-dot output)
    no_drop_no_rope(p);
    p.rope_T = T; p.rope_hs = head_dim;
    const int prof = obte_prof_begin(st, prof_kind(g, 7), g->M, g->N, g->K);   // (recorded as the dy W product it is)
    const int rc = obte_gemm_v7_launch(p, true, false, OBTE_EPI_ROWDOT, st);
    obte_prof_end(prof, st);
    return rc;
}

// Grouped launch (see gemm_v3_group_kernel).  Each problem: any layout, epilogue NONE or ADD, K >= 128; or ACC32 in its one layout.
extern "C" int obte_gemm_grouped_bf16(const obte_gemm_args* gs, int count, obte_stream s) {
    OBTE_REQUIRE(gs && count >= 1 && count <= GROUP_MAX, "obte_gemm_grouped_bf16: count must be 1..%d", GROUP_MAX);
    GroupParams gp;
    memset(&gp, 0, sizeof(gp));
    hipStream_t st = (hipStream_t)s;
    int wg = 0, class0 = 0;
    bool in_class0 = true;
    double flop = 0.0;
    for (int i = 0; i < count; ++i) {
        const obte_gemm_args* g = gs + i;
        OBTE_REQUIRE(g->epilogue == OBTE_EPI_NONE || g->epilogue == OBTE_EPI_ADD || g->epilogue == OBTE_EPI_ACC32, "obte_gemm_grouped_bf16: epilogue must be NONE or ADD (or ACC32, the fp32 sum of a weight gradient)");
        { const int vrc = validate_args(g); if (vrc != OBTE_OK) return vrc; }
        OBTE_REQUIRE(g->K >= 128, "obte_gemm_grouped_bf16: K must be >= 128 (K=%lld)", (long long)g->K);
        OBTE_REQUIRE(cdiv64(g->M, BM) * cdiv64(g->N, 256) < (1ll << 24), "obte_gemm_grouped_bf16: too many tiles");
        GemmParams& p = gp.g[i];
        fill_params(g, nullptr, Plan{3, 256, 1}, p);
        no_drop_no_rope(p);
        if (g->epilogue == OBTE_EPI_NONE) p.aux = nullptr;
        gp.layout[i] = g->epilogue == OBTE_EPI_ACC32 ? 4 : layout_of(g);   // (ACC32: the weight-gradient layout with the fp32 epilogue)
        gp.first_wg[i] = wg;
        wg += p.tiles_m * p.tiles_n;
        if (in_class0 && p.k_per_split == gp.g[0].k_per_split) class0 = wg; else in_class0 = false;
        flop += 2.0 * (double)g->M * (double)g->N * (double)g->K;
    }
    for (int i = count; i <= GROUP_MAX; ++i) gp.first_wg[i] = wg;
    for (int i = count; i < GROUP_MAX; ++i) { gp.g[i] = gp.g[0]; gp.layout[i] = gp.layout[0]; }   // never selected
    gp.n_class0 = (class0 < wg && class0 % 8 == 0 && (wg - class0) % 8 == 0) ? class0 : 0;
    // profiler record: one entry; d0 chosen so that 2*d0*d1*d2 is the group's total FLOP
    const int prof = obte_prof_begin(st, prof_kind(gs, 3, gs + count - 1), (int64_t)(flop / (2.0 * (double)gs[0].N * (double)gs[0].K) + 0.5), gs[0].N, gs[0].K);
    const int rc = obte_gemm_group_launch(gp, st);
    obte_prof_end(prof, st);
    return rc;
}
