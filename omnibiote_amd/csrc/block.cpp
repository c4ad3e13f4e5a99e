// Host-side sequencing of one transformer block (training/model.py:170-181): a single C call enqueues every
// kernel of the block's forward (or backward) on the caller's stream, so the Python layer crosses the
// boundary once per block and pass.  Pre-LN residual wiring:
//     x1 = x  + c_proj(attn(rope(c_attn(ln_1(x)))))        out = x1 + mlp.c_proj(gelu(c_fc(ln_2(x1))))
// The residual adds live in the GEMM epilogues, GELU in c_fc's epilogue, GELU' in the mlp.c_proj dgrad epilogue,
// the residual-gradient adds in the LayerNorm backward kernels, inverse RoPE in the attention backward epilogue.
//
// A call takes one of three forms (BlockForm, resolve() below; n = n_out_rows wanted rows, M = B T positions):
//
//                  full (out_rows null)               rows, key ranges / no mask            rows, dense mask
//   c_attn         one product, RoPE in epilogue      k, v thirds on M rows + RoPE pass;    as full
//                                                     q third on the n rows + RoPE pass
//   attention      M queries                          n queries (obte_attn_*_rows)          as full, output rows gathered
//   c_proj, MLP    M rows, dropout in the epilogues   n rows; c_proj's dropout a pass of its own (mask elements (rows[i], c))
//   backward       dy_attn with the row-dot           c_proj and c_attn's q third on n      c_proj on n rows, d(attention output)
//                  epilogue; c_attn from the whole    rows, c_attn by thirds; dh1 =         scattered; attention and c_attn as
//                  dqkv                               [dK dV] W_kv + rows(dQ W_q)           full
//   weight grads   all four + dh1 in one grouped      each its own launch; the MLP half's two as one pair where n >= 256
//                  launch where that fills the chip
//   regions        as named                           y: Q of the rows; x1: the rows' attention output; x1r: ln_1(x) rows, then
//                                                     x, then x1 of the rows; h2 / hpre before ln_2 / c_fc write them: c_proj
//                                                     staging and split-K workspace.  Dense mask: y is the full output, x1
//                                                     its gathered rows, x1r holds x / x1 rows only
//   workspace      dym / dym2: dy and dx1 under       dyattn: dx1 rows, then ln_1(x) rows (dense mask: then the full d(attention
//                  their dropout masks                output)); dym: d(attention output) rows, then dQ W_q rows; dym2: masked dx1
//                                                     rows, then dQ rows
// The reuses are named members of ActLayout / WsLayout, each with the moment from which its region is free.
// obte_block_fwd_infer is the full form's forward for a caller who will never run the backward: the same products, nothing kept
// (InferLayout: seven [M, C] units instead of fifteen), c_fc's activation without its derivative.  obte_block_fwd_prefill is that call with
// the rotated keys and the values also copied into a layer's key/value cache, obte_block_decode the same sequence on ONE new position per
// row whose attention reads that cache (csrc/attention_decode.hip), obte_block_extend on n new positions per row (csrc/attention_extend.hip),
// obte_block_decode_shared the decode step of P groups of rows over a prefix cache per group and a suffix cache per row
// (csrc/attention_shared.hip): the five share infer_sequence() below.
#include "common.h"

namespace {

inline int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }

// The activation buffer of one block: typed pointers to its regions, laid out from `base` (null: only `total` means anything).
// The rows form reuses regions under other roles; every reuse has its NAME here, with the moment from which the region is free.
struct ActLayout {
    float *mean1, *rstd1, *lse, *mean2, *rstd2;
    obte_bf16 *h1, *qkv, *y, *x1, *h2, *hpre, *hact, *x1r;
    int32_t *r_off, *r_boff, *r_pos, *r_kr, *r_qb, *r_inv;   // the tables of obte_attn_rows_prep (r_inv: written by it, no reader left; it
                                                              // stays so that neither the buffer's size nor that launch changes)
    uint32_t* dropbits;
    int64_t total;
    obte_bf16* rows_q;          // = y: Q of the wanted rows (the attention's queries are those rows: the full output is never formed)
    obte_bf16* rows_attn_out;   // = x1: the attention output at the wanted rows, kept for the backward (the full x1 is never formed)
    obte_bf16* rows_h1;         // = x1r: ln_1(x) at the wanted rows, read by the q product before ...
    obte_bf16* rows_x1;         // = x1r: ... x, then x1 at the wanted rows (the backward reads it)
    obte_bf16* proj_stage;      // = h2: the rows' projection before its dropout (ln_2 writes h2 after)
    void* splitk_ws;            // = hpre: split-K workspace of the rows' q and projection products (c_fc writes hpre after)
    int64_t splitk_ws_bytes;
    // with_bits: the attention dropout's keep bits (B H ceil(T/32) T words: 134 MB per block at B = 8, T = 4096) are part of the
    // buffer only when dropout is on; they are the LAST region, so every other offset is the same either way
    ActLayout(int64_t B, int64_t T, int C, int H, bool with_bits = true, const void* base = nullptr) {
        const int64_t M = B * T;
        uintptr_t o = (uintptr_t)base;
        auto take = [&](int64_t bytes) { void* r = (void*)o; o += align256(bytes); return r; };
        mean1 = (float*)take(M * 4); rstd1 = (float*)take(M * 4);
        h1 = (obte_bf16*)take(M * C * 2);
        qkv = (obte_bf16*)take(M * 3 * C * 2);
        lse = (float*)take(B * H * T * 4);
        y = (obte_bf16*)take(M * C * 2); x1 = (obte_bf16*)take(M * C * 2);
        mean2 = (float*)take(M * 4); rstd2 = (float*)take(M * 4);
        h2 = (obte_bf16*)take(M * C * 2);
        hpre = (obte_bf16*)take(M * 4 * C * 2); hact = (obte_bf16*)take(M * 4 * C * 2);
        x1r = (obte_bf16*)take(M * C * 2);      // rows form (obte_block_desc::out_rows): x1 at the wanted positions
        r_off = (int32_t*)take((B + 1) * 4); r_boff = (int32_t*)take((B + 1) * 4); r_pos = (int32_t*)take(M * 4);
        r_kr = (int32_t*)take(M * 8); r_qb = (int32_t*)take(M * 8); r_inv = (int32_t*)take(M * 4);
        dropbits = (uint32_t*)take(with_bits ? obte_attn_drop_bits_bytes(B, T, H) : 0);   // attention dropout: the forward's keep bits for the backward
        total = (int64_t)(o - (uintptr_t)base);
        rows_q = y; rows_attn_out = x1; rows_h1 = rows_x1 = x1r; proj_stage = h2;
        splitk_ws = hpre; splitk_ws_bytes = M * 4 * C * 2;
    }
};

// The same for the backward's workspace.
struct WsLayout {
    obte_bf16 *dhpre, *dh, *dx1, *dyattn, *dqkv, *dym, *dym2;
    float *delta, *lnws;
    void *gemmws, *attnws;   // null where the byte count is 0
    int64_t gemmws_bytes, attnws_bytes, total;
    obte_bf16* dx1_rows;          // = dyattn: d x1 at the wanted rows, until the projection's two products have read it; then
    obte_bf16* h1_rows;           // = dyattn: ln_1(x) at the wanted rows, for dW_q
    obte_bf16* dy_attn_rows;      // = dym: d(attention output) at the wanted rows (the MLP half's products were dym's last readers; a dense
                                  //   mask: scattered into dyattn once both of the projection's products have read dx1_rows there); then
    obte_bf16* dh1_rows;          // = dym: dQ W_q at the wanted rows (the attention backward has read its d_o)
    obte_bf16* dx1_rows_masked;   // = dym2: d x1 at the wanted rows under the projection's mask, until both products have read it; then
    obte_bf16* dq_rows;           // = dym2: dQ of the wanted rows
    WsLayout(int64_t B, int64_t T, int C, int H, void* base = nullptr) {
        const int64_t M = B * T;
        uintptr_t o = (uintptr_t)base;
        auto take = [&](int64_t bytes) { void* r = (void*)o; o += align256(bytes); return r; };
        dhpre = (obte_bf16*)take(M * 4 * C * 2);
        dh = (obte_bf16*)take(M * C * 2);       // dh2, later dh1
        dx1 = (obte_bf16*)take(M * C * 2);
        dyattn = (obte_bf16*)take(M * C * 2);
        dqkv = (obte_bf16*)take(M * 3 * C * 2);
        delta = (float*)take(B * H * T * 4);
        lnws = (float*)take((int64_t)obte_layernorm_bwd_ws_rows() * C * 4);
        dym = (obte_bf16*)take(M * C * 2);      // dropout-masked copies of the two incoming gradients, dy and dx1 (only touched when dropout_p > 0);
        dym2 = (obte_bf16*)take(M * C * 2);     // two buffers: both stay live until the grouped weight-gradient launch at the end
        gemmws_bytes = 0;
        const int64_t shapes[4][2] = {{C, 4 * C}, {4 * C, C}, {C, C}, {3 * C, C}};   // the four weight gradients
        for (auto& sh : shapes) {
            const int64_t b = obte_gemm_workspace_bytes(sh[0], sh[1], M);
            if (b > gemmws_bytes) gemmws_bytes = b;
        }
        gemmws = take(gemmws_bytes > 0 ? gemmws_bytes : 256);
        attnws_bytes = obte_attn_bwd_ws_bytes(B, T, H, C / H);   // the one-kernel attention backward's dQ contributions (0: not applicable)
        attnws = take(attnws_bytes > 0 ? attnws_bytes : 256);
        total = (int64_t)(o - (uintptr_t)base);
        if (gemmws_bytes == 0) gemmws = nullptr;
        if (attnws_bytes == 0) attnws = nullptr;
        dx1_rows = h1_rows = dyattn; dy_attn_rows = dh1_rows = dym; dx1_rows_masked = dq_rows = dym2;
    }
};

// The workspace of a forward nobody will differentiate (obte_block_fwd_infer): nothing outlives the call, so a region is reused as soon
// as its last reader has been enqueued — seven [M, C] bf16 units and the small fp32 rows, against the fifteen of ActLayout.
struct InferLayout {
    obte_bf16 *qkv, *h1, *att, *x1;
    float *mean, *rstd, *lse;   // written by the LayerNorm and attention kernels, read by nobody; ln_2 overwrites ln_1's statistics
    int64_t total;
    obte_bf16* hact;            // = qkv: gelu(c_fc) [M, 4C] over the [M, 3C] qkv and the unit behind it (the attention was qkv's last reader)
    obte_bf16* h2;              // = h1: ln_2(x1) (c_attn was h1's last reader)
    InferLayout(int64_t B, int64_t T, int C, int H, const void* base = nullptr) {
        const int64_t M = B * T;
        uintptr_t o = (uintptr_t)base;
        auto take = [&](int64_t bytes) { void* r = (void*)o; o += align256(bytes); return r; };
        qkv = (obte_bf16*)take(M * 4 * C * 2);
        h1 = (obte_bf16*)take(M * C * 2);
        att = (obte_bf16*)take(M * C * 2);
        x1 = (obte_bf16*)take(M * C * 2);
        mean = (float*)take(M * 4); rstd = (float*)take(M * 4);
        lse = (float*)take(B * H * T * 4);
        total = (int64_t)(o - (uintptr_t)base);
        hact = qkv; h2 = h1;
    }
};

// ---- products of the block: x W^T, dy W and a^T b (row-major operands), the rest of obte_gemm_args set by name at the call ------------
obte_gemm_args product(const obte_bf16* a, const obte_bf16* b, obte_bf16* out, int64_t m, int64_t n, int64_t k, int ak, int bk) {
    obte_gemm_args g = {};
    g.a = a; g.b = b; g.d = out; g.M = m; g.N = n; g.K = k;
    g.lda = ak ? k : m; g.ldb = bk ? k : n; g.ldd = n;
    g.a_kmajor = ak; g.b_kmajor = bk; g.epilogue = OBTE_EPI_NONE; g.alpha = 1.0f;
    return g;
}
// out[m, n] = x[m, k] w[n, k]^T
obte_gemm_args xWt(const obte_bf16* x, const obte_bf16* w, obte_bf16* out, int64_t m, int64_t n, int64_t k) { return product(x, w, out, m, n, k, 1, 1); }
// out[m, n] = dy[m, k] w[k, n]
obte_gemm_args dyW(const obte_bf16* dy, const obte_bf16* w, obte_bf16* out, int64_t m, int64_t n, int64_t k) { return product(dy, w, out, m, n, k, 1, 0); }
// How one weight gradient is delivered: overwritten, accumulated in place in bf16, or summed into the caller's fp32 buffer of the weight's
// shape over the passes of a step (acc32 + mode OBTE_ACC32_*: dw is then written by the last pass only)
struct Wgrad { obte_bf16* dw; bool accumulate; float* acc32; int mode; };
// dw[m, n] (+)= a[k, m]^T b[k, n]: a weight gradient over k rows; row0: the first of the weight's rows this product forms (c_attn by thirds)
obte_gemm_args aTb(const obte_bf16* a, const obte_bf16* b, const Wgrad& w, int64_t m, int64_t n, int64_t k, int64_t row0 = 0) {
    obte_gemm_args g = product(a, b, w.dw ? w.dw + row0 * n : nullptr, m, n, k, 0, 0);
    if (w.mode) { g.epilogue = OBTE_EPI_ACC32; g.acc32 = w.acc32 + row0 * n; g.acc32_mode = w.mode; }
    else if (w.accumulate) { g.epilogue = OBTE_EPI_ADD; g.aux = g.d; }
    return g;
}
// out = resid + [dropout under (seed, site)] (the product): the residual adds of the forward
obte_gemm_args plus_residual(obte_gemm_args g, const obte_bf16* resid, float p = 0.f, uint64_t seed = 0, int site = 0) {
    g.epilogue = OBTE_EPI_ADD; g.aux = resid;
    if (p > 0.f) { g.epilogue = OBTE_EPI_ADD_DROPOUT; g.dropout_p = p; g.dropout_seed = seed; g.dropout_site = site; }
    return g;
}
int run(const obte_gemm_args& g, obte_stream s, void* ws = nullptr, int64_t ws_bytes = 0) { return obte_gemm_bf16_ws(&g, ws, ws_bytes, s); }

// dropout sites of one block (csrc/common.h OBTE_SITE_*): 1 attention probabilities, 2 attention c_proj, 3 MLP c_proj
enum { SITE_RESID = 2, SITE_MLP = 3 };

int check_desc(const char* who, const obte_block_desc* d) {
    OBTE_REQUIRE(d, "%s: null descriptor", who);
    OBTE_REQUIRE(d->B > 0 && d->T > 0 && d->n_head > 0 && d->n_embd > 0, "%s: bad shape", who);
    OBTE_REQUIRE(d->n_embd % d->n_head == 0, "%s: n_embd %% n_head != 0", who);
    const int hs = d->n_embd / d->n_head;
    OBTE_REQUIRE(hs == 64 || hs == 128, "%s: head size %d unsupported by the HIP path (64 or 128)", who, hs);
    OBTE_REQUIRE(d->n_embd % 64 == 0 && d->n_embd <= 4096, "%s: n_embd must be a multiple of 64 and <= 4096", who);
    OBTE_REQUIRE(d->ln1_w && d->attn_w && d->proj_w && d->ln2_w && d->fc_w && d->mlp_w && d->rope_cos && d->rope_sin,
                 "%s: null parameter", who);
    OBTE_REQUIRE(d->dropout_p >= 0.f && d->dropout_p < 1.f, "%s: dropout p must be in [0,1)", who);
    OBTE_REQUIRE((d->out_rows == nullptr) == (d->n_out_rows == 0) && d->n_out_rows >= 0 && d->n_out_rows <= d->B * d->T, "%s: out_rows / n_out_rows inconsistent", who);
    return OBTE_OK;
}

#define TRY(x) do { int rc_ = (x); if (rc_ != OBTE_OK) return rc_; } while (0)

// ---- the form of one call: every decision of the forward and the backward, taken once ------------------------------------------------
// The backward reads the regions the forward filled according to these flags, so both start from resolve(d) and derive nothing else.
struct BlockForm {
    int64_t M, Mm;     // positions of the block; positions the MLP half and (rows form) the attention projection run on
    bool drop;         // dropout on
    bool rows;         // rows form (obte_block_desc::out_rows, the model's last block)
    bool rows_attn;    // rows form without a dense mask: the attention's queries and c_attn's q third at the wanted rows only
    bool grouped;      // backward, not the rows form: ONE grouped launch for the four weight gradients and dh1 = dqkv W_attn
    bool pair_mlp;     // backward, rows form: the MLP half's two weight gradients (K = Mm) as one launch of their own
};

// The four weight gradients of a block go out as ONE grouped launch (obte_gemm_grouped_bf16) when their 256x256 tiles
// fill the chip reasonably (>= 70 % of the CU slots of the rounds they need); tiny widths keep the per-matrix split-K
// launches.  OBTE_GROUPED_WGRAD=0/1 overrides (tests reach both forms at small sizes: read per call).
bool use_grouped_wgrad(int C, int64_t M) {
    const char* e = getenv("OBTE_GROUPED_WGRAD");
    if (e && (e[0] == '0' || e[0] == '1')) return e[0] == '1' && M >= 128;
    if (M < 1024) return false;
    auto t = [](int64_t m, int64_t n) { return ((m + 255) / 256) * ((n + 255) / 256); };
    const int64_t tiles = t(C, 4 * C) + t(4 * C, C) + t(C, C) + t(3 * C, C);
    const int64_t rounds = (tiles + 255) / 256;
    return tiles * 10 >= rounds * 256 * 7;
}

BlockForm resolve(const obte_block_desc* d) {
    BlockForm f = {};
    f.M = d->B * d->T;
    f.drop = d->dropout_p > 0.f;
    f.rows = d->out_rows != nullptr;
    f.Mm = f.rows ? d->n_out_rows : f.M;
    f.rows_attn = f.rows && d->mask == nullptr;
    // Rows form: the attention half's two weight gradients and dh1 are an unbalanced group (686 us against ~430 as three launches with
    // their tuned plans: DESIGN.md 13.4), so each is its own launch; the MLP half's two contract over the Mm wanted rows and pair up
    // when those are enough for the grouped kernel's K.
    const bool grouped_ok = use_grouped_wgrad(d->n_embd, f.M);
    f.grouped = grouped_ok && !f.rows;
    f.pair_mlp = grouped_ok && f.rows && f.Mm >= 256;
    return f;
}

obte_attn_rows attn_rows_tables(const obte_block_desc* d, const ActLayout& a) {
    obte_attn_rows ar = {};
    ar.q_off = a.r_off; ar.q_blk_off = a.r_boff; ar.q_pos = a.r_pos; ar.n = d->n_out_rows;
    if (d->key_ranges) { ar.key_ranges = a.r_kr; ar.query_bounds = a.r_qb; }
    return ar;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------

// attention with its queries at the wanted rows: q = ln_1(x) W_q^T formed for those rows and rotated at their positions, the output
// where the projection expects it
int fwd_attention_rows(const obte_block_desc* d, const BlockForm& f, const ActLayout& a, obte_attn_fwd_args af, obte_stream s) {
    const int C = d->n_embd;
    const obte_attn_rows ar = attn_rows_tables(d, a);   // (filled once per call: the backward reads them)
    TRY(obte_attn_rows_prep(d->out_rows, d->n_out_rows, d->B, d->T, d->key_ranges, d->query_bounds, a.r_off, a.r_boff, a.r_pos, a.r_kr, a.r_qb, a.r_inv, s));
    TRY(obte_rows_gather_bf16(a.h1, d->out_rows, a.rows_h1, f.Mm, f.M, C, s));
    TRY(run(xWt(a.rows_h1, d->attn_w, a.rows_q, f.Mm, C, C), s, a.splitk_ws, a.splitk_ws_bytes));
    TRY(obte_rope_cols_bf16(a.rows_q, C, C, d->rope_cos, d->rope_sin, f.Mm, d->T, a.r_pos, af.head_dim, s));
    af.o = a.rows_attn_out;
    return obte_attn_fwd_rows(&af, &ar, a.rows_q, s);
}

// ln_1, c_attn with RoPE, attention
int fwd_attention(const obte_block_desc* d, const BlockForm& f, const ActLayout& a, const obte_bf16* x, obte_stream s) {
    const int C = d->n_embd, H = d->n_head, hs = C / H;
    TRY(obte_layernorm_fwd(x, d->ln1_w, a.h1, a.mean1, a.rstd1, f.M, C, 1e-5f, s));
    if (f.rows_attn) {   // c_attn by its output thirds: W_attn's rows C .. 3C-1 make k and v for every position (the k third rotated in
                         // place), rows 0 .. C-1 q for the wanted rows; RoPE as its own passes with the arithmetic of the fused epilogue
        obte_gemm_args g = xWt(a.h1, d->attn_w + (int64_t)C * C, a.qkv + C, f.M, 2 * C, C);
        g.ldd = 3 * C;
        TRY(run(g, s));
        TRY(obte_rope_cols_bf16(a.qkv + C, 3 * (int64_t)C, C, d->rope_cos, d->rope_sin, f.M, d->T, nullptr, hs, s));
    } else {   // c_attn with RoPE on its q and k thirds fused in the epilogue (model.py:102-108)
        obte_gemm_args g = xWt(a.h1, d->attn_w, a.qkv, f.M, 3 * C, C);
        g.epilogue = OBTE_EPI_ROPE_QK; g.rope_cos = d->rope_cos; g.rope_sin = d->rope_sin; g.rope_T = d->T; g.rope_head_dim = hs;
        TRY(run(g, s));
    }
    obte_attn_fwd_args af = {};
    af.qkv = a.qkv; af.o = a.y; af.lse = a.lse; af.key_ranges = d->key_ranges; af.mask = d->mask;
    af.mask_sb = d->mask_sb; af.mask_sh = d->mask_sh; af.mask_sq = d->mask_sq; af.ranges_exact = d->ranges_exact;
    af.B = d->B; af.T = d->T; af.n_head = H; af.head_dim = hs; af.scale = 8.0f / (float)C;  // model.py:119
    af.dropout_p = d->dropout_p; af.dropout_seed = d->dropout_seed;
    if (f.rows_attn) return fwd_attention_rows(d, f, a, af, s);   // (no keep bits: a gathered query set hashes in both passes)
    if (f.drop) {   // the keep bits for the backward; words of key tiles the forward skips (pairs the mask excludes) stay defined whoever reads them
        af.drop_bits = a.dropbits;
        if (hipMemsetAsync(af.drop_bits, 0, (size_t)obte_attn_drop_bits_bytes(d->B, d->T, H), (hipStream_t)s) != hipSuccess) {
            obte_set_error("obte_block_fwd: memset of the dropout keep bits failed");
            return OBTE_ELAUNCH;
        }
    }
    return obte_attn_fwd(&af, s);
}

// x1 = x + dropout(y W_proj^T) for the wanted rows alone (per-position arithmetic, same results there): the attention output and the
// block input gathered
int fwd_proj_rows(const obte_block_desc* d, const BlockForm& f, const ActLayout& a, const obte_bf16* x, obte_stream s) {
    const int C = d->n_embd;
    TRY(obte_rows_gather_bf16(x, d->out_rows, a.rows_x1, f.Mm, f.M, C, s));
    if (!f.rows_attn) TRY(obte_rows_gather_bf16(a.y, d->out_rows, a.rows_attn_out, f.Mm, f.M, C, s));   // (a dense mask; else the attention wrote the wanted rows there itself)
    if (f.drop) {   // the mask of site 2 is defined on the whole activation — element (rows[i], c) for gathered row i — so not in the epilogue
        TRY(run(xWt(a.rows_attn_out, d->proj_w, a.proj_stage, f.Mm, C, C), s, a.splitk_ws, a.splitk_ws_bytes));
        return obte_dropout_rows_bf16(a.proj_stage, a.rows_x1, a.rows_x1, d->out_rows, f.Mm, C, d->dropout_p, d->dropout_seed, SITE_RESID, s);
    }
    return run(plus_residual(xWt(a.rows_attn_out, d->proj_w, a.rows_x1, f.Mm, C, C), a.rows_x1), s, a.splitk_ws, a.splitk_ws_bytes);
}

// out = x1 + dropout(gelu(ln_2(x1) W_fc^T) W_mlp^T) on the Mm rows of x1m
int fwd_mlp(const obte_block_desc* d, const BlockForm& f, const ActLayout& a, const obte_bf16* x1m, obte_bf16* y_out, obte_stream s) {
    const int C = d->n_embd;
    TRY(obte_layernorm_fwd(x1m, d->ln2_w, a.h2, a.mean2, a.rstd2, f.Mm, C, 1e-5f, s));
    obte_gemm_args fc = xWt(a.h2, d->fc_w, a.hpre, f.Mm, 4 * C, C);
    fc.epilogue = OBTE_EPI_GELU; fc.d2 = a.hact;
    TRY(run(fc, s));
    // rows form: [Mm, C] over K = 4C is a handful of tiles — split-K, with the tail of the (M-row) hpre region its Mm rows leave unused as workspace
    const int64_t used = align256(f.Mm * 4 * C * 2);
    int64_t tail_bytes = f.M * 4 * C * 2 - used;
    if (!f.rows || tail_bytes < (int64_t)(2 * f.Mm * C * 4)) tail_bytes = 0;
    void* tail = tail_bytes ? (char*)a.hpre + used : nullptr;
    return run(plus_residual(xWt(a.hact, d->mlp_w, y_out, f.Mm, C, 4 * C), x1m, d->dropout_p, d->dropout_seed, SITE_MLP), s, tail, tail_bytes);
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------

struct Grads {   // the caller's six gradient buffers and how they are written
    obte_bf16 *ln1_w, *ln2_w;
    Wgrad attn_w, proj_w, fc_w, mlp_w;   // the four matrices: overwritten, dW += ... straight into the .grad buffers, or summed in fp32
    int acc_ln;    // the two LayerNorm weights accumulated in place
};

// dx = resid + LN'(dh) over `rows` rows, dw by the descriptor's mode (fp32 partials across micro-batches, or the workspace);
// masked != null: dropout(dx) under (seed, site) written there as well
int ln_bwd(const obte_block_desc* d, const Grads& g, const WsLayout& w, const obte_bf16* dh, const obte_bf16* x, const obte_bf16* weight,
           const float* mean, const float* rstd, const obte_bf16* resid, obte_bf16* dx, obte_bf16* dw, float* partials, int64_t rows,
           obte_stream s, obte_bf16* masked = nullptr, uint64_t seed = 0, int site = 0) {
    const int C = d->n_embd, lnp = d->ln_partial_mode;
    if (masked) return obte_layernorm_bwd_dropout(dh, x, weight, mean, rstd, resid, dx, masked, dw, lnp ? partials : w.lnws, rows, C, lnp, g.acc_ln,
                                                  d->dropout_p, seed, site, s);
    if (lnp) return obte_layernorm_bwd_partial(dh, x, weight, mean, rstd, resid, dx, dw, partials, rows, C, lnp, s);
    return obte_layernorm_bwd_acc(dh, x, weight, mean, rstd, resid, dx, dw, w.lnws, rows, C, g.acc_ln, s);
}

// out = x1 + dropout(hact W_mlp^T): dhpre, dh2 (in w.dh) and, unless a grouped launch takes them, dW_mlp and dW_fc.
// *dy_mlp: dy under the (seed, site 3) mask — [Mm, C], element (i, c) of the compact output in the rows form, as in the forward
int bwd_mlp(const obte_block_desc* d, const BlockForm& f, const ActLayout& a, const WsLayout& w, const Grads& g, const obte_bf16* dy, const obte_bf16** dy_mlp, obte_stream s) {
    const int C = d->n_embd;
    *dy_mlp = dy;
    if (f.drop && d->dy_masked) {   // handed over by the block above: its last LayerNorm backward wrote dropout(dx) under this block's mask
        *dy_mlp = d->dy_masked;
    } else if (f.drop) {
        TRY(obte_dropout_bf16(dy, w.dym, f.Mm * C, C, d->dropout_p, d->dropout_seed, SITE_MLP, s));
        *dy_mlp = w.dym;
    }
    obte_gemm_args dgelu = dyW(*dy_mlp, d->mlp_w, w.dhpre, f.Mm, 4 * C, C);   // dhpre = (dy W_mlp) * gelu'(h): hpre holds the derivative
    dgelu.epilogue = OBTE_EPI_GELU_BWD; dgelu.aux = a.hpre;
    TRY(run(dgelu, s));
    const obte_gemm_args dw_mlp = aTb(*dy_mlp, a.hact, g.mlp_w, C, 4 * C, f.Mm);   // dW_mlp = dy^T hact
    const obte_gemm_args dw_fc = aTb(w.dhpre, a.h2, g.fc_w, 4 * C, C, f.Mm);       // dW_fc = dhpre^T h2
    const bool own = !f.grouped && !f.pair_mlp;
    if (own) TRY(run(dw_mlp, s, w.gemmws, w.gemmws_bytes));
    TRY(run(dyW(w.dhpre, d->fc_w, w.dh, f.Mm, C, 4 * C), s, f.rows ? w.gemmws : nullptr, f.rows ? w.gemmws_bytes : 0));   // dh2 = dhpre W_fc (rows form: few tiles over K = 4C, split-K)
    if (own) TRY(run(dw_fc, s, w.gemmws, w.gemmws_bytes));
    if (f.pair_mlp) {
        const obte_gemm_args pair[2] = {dw_fc, dw_mlp};
        TRY(obte_gemm_grouped_bf16(pair, 2, s));
    }
    return OBTE_OK;
}

// dx1 = dy + LN2'(dh2), then the attention projection: x1 = x + dropout(y W_proj^T), so it sees dx1 under the (seed, site 2) mask
// (*dx1_proj) — with dropout on, the LayerNorm backward writes that masked copy beside dx1.  dy_attn = dx1 W_proj goes, where
// structure 7 takes the shape, with the softmax backward's delta = rowsum(dy_attn o y) formed in its epilogue (*delta_ready; the
// attention backward's prep launch would otherwise read both tensors again to form it); dW_proj = dx1^T y unless grouped below
int bwd_ln2_proj_full(const obte_block_desc* d, const BlockForm& f, const ActLayout& a, const WsLayout& w, const Grads& g, const obte_bf16* dy,
                      const obte_bf16** dx1_proj, bool* delta_ready, obte_stream s) {
    const int C = d->n_embd;
    TRY(ln_bwd(d, g, w, w.dh, a.x1, d->ln2_w, a.mean2, a.rstd2, dy, w.dx1, g.ln2_w, d->ln2_partials, f.M, s,
               f.drop ? w.dym2 : nullptr, d->dropout_seed, SITE_RESID));
    *dx1_proj = f.drop ? w.dym2 : w.dx1;
    const obte_gemm_args dgrad = dyW(*dx1_proj, d->proj_w, w.dyattn, f.M, C, C);
    const int rc = obte_gemm_rowdot_bf16(&dgrad, a.y, w.delta, d->T, C / d->n_head, s);
    if (rc == OBTE_OK) *delta_ready = true;
    else if (rc == OBTE_ROWDOT_NOT_TAKEN) TRY(obte_gemm_bf16(&dgrad, s));
    else return rc;
    if (!f.grouped) TRY(run(aTb(*dx1_proj, a.y, g.proj_w, C, C, f.M), s, w.gemmws, w.gemmws_bytes));
    return OBTE_OK;
}

// rows form: d x1 at the wanted rows, scattered into zeros for ln_1; the projection's two gradients contract over / are formed for
// those rows only.  A dense mask: d(attention output) scattered for the full attention backward.
int bwd_ln2_proj_rows(const obte_block_desc* d, const BlockForm& f, const ActLayout& a, const WsLayout& w, const Grads& g, const obte_bf16* dy, obte_stream s) {
    const int C = d->n_embd;
    TRY(ln_bwd(d, g, w, w.dh, a.rows_x1, d->ln2_w, a.mean2, a.rstd2, dy, w.dx1_rows, g.ln2_w, d->ln2_partials, f.Mm, s));
    TRY(obte_rows_scatter_bf16(w.dx1_rows, d->out_rows, w.dx1, f.Mm, f.M, C, s));
    const obte_bf16* dxp = w.dx1_rows;
    if (f.drop) {   // under the projection's mask: element (rows[i], c)
        TRY(obte_dropout_rows_bf16(w.dx1_rows, nullptr, w.dx1_rows_masked, d->out_rows, f.Mm, C, d->dropout_p, d->dropout_seed, SITE_RESID, s));
        dxp = w.dx1_rows_masked;
    }
    TRY(run(dyW(dxp, d->proj_w, w.dy_attn_rows, f.Mm, C, C), s, w.gemmws, w.gemmws_bytes));
    TRY(run(aTb(dxp, a.rows_attn_out, g.proj_w, C, C, f.Mm), s, w.gemmws, w.gemmws_bytes));   // dW_proj = dx1^T y over the wanted rows
    if (!f.rows_attn) TRY(obte_rows_scatter_bf16(w.dy_attn_rows, d->out_rows, w.dyattn, f.Mm, f.M, C, s));   // (dx1_rows, in dyattn, has been read by both products)
    return OBTE_OK;
}

// attention with the queries at the wanted rows: everything on the query side is the gathered set; then c_attn's backward
// by thirds: dK / dV of every position against W's k and v rows, dQ of the wanted rows against its q rows
int bwd_attention_rows(const obte_block_desc* d, const BlockForm& f, const ActLayout& a, const WsLayout& w, const Grads& g, obte_attn_bwd_args ab, obte_stream s) {
    const int C = d->n_embd;
    const obte_attn_rows ar = attn_rows_tables(d, a);
    ab.o = a.rows_attn_out; ab.d_o = w.dy_attn_rows;
    TRY(obte_attn_bwd_rows(&ab, &ar, a.rows_q, w.dq_rows, s));
    const obte_bf16* dkv = w.dqkv + C;
    obte_gemm_args dh1 = dyW(dkv, d->attn_w + (int64_t)C * C, w.dh, f.M, C, 2 * C);   // dh1 = [dK dV] W_kv
    dh1.lda = 3 * C;
    TRY(run(dh1, s));
    TRY(run(dyW(w.dq_rows, d->attn_w, w.dh1_rows, f.Mm, C, C), s, w.gemmws, w.gemmws_bytes));   //       + dQ W_q at the wanted rows
    TRY(obte_rows_add_bf16(w.dh1_rows, d->out_rows, w.dh, f.Mm, C, s));
    TRY(obte_rows_gather_bf16(a.h1, d->out_rows, w.h1_rows, f.Mm, f.M, C, s));
    obte_gemm_args dw_kv = aTb(dkv, a.h1, g.attn_w, 2 * C, C, f.M, C);   // dW_kv = [dK dV]^T ln_1(x)
    dw_kv.lda = 3 * C;
    TRY(run(dw_kv, s, w.gemmws, w.gemmws_bytes));
    return run(aTb(w.dq_rows, w.h1_rows, g.attn_w, C, C, f.Mm), s, w.gemmws, w.gemmws_bytes);   // dW_q = dQ^T ln_1(x) over the wanted rows
}

// dqkv from d(attention output) (inverse RoPE in the epilogue)
int bwd_attention(const obte_block_desc* d, const BlockForm& f, const ActLayout& a, const WsLayout& w, const Grads& g, bool delta_ready, obte_stream s) {
    const int C = d->n_embd, H = d->n_head;
    obte_attn_bwd_args ab = {};
    ab.qkv = a.qkv; ab.o = a.y; ab.d_o = w.dyattn; ab.lse = a.lse; ab.delta = w.delta; ab.dqkv = w.dqkv;
    ab.rope_cos = d->rope_cos; ab.rope_sin = d->rope_sin;
    ab.key_ranges = d->key_ranges; ab.mask = d->mask; ab.mask_sb = d->mask_sb; ab.mask_sh = d->mask_sh; ab.mask_sq = d->mask_sq;
    ab.query_bounds = d->query_bounds; ab.ranges_exact = d->ranges_exact;
    ab.B = d->B; ab.T = d->T; ab.n_head = H; ab.head_dim = C / H; ab.scale = 8.0f / (float)C;
    ab.dropout_p = d->dropout_p; ab.dropout_seed = d->dropout_seed;
    ab.drop_bits = (f.drop && !f.rows_attn) ? a.dropbits : nullptr;
    if (w.attnws) { ab.ws = w.attnws; ab.ws_bytes = w.attnws_bytes; }
    if (f.rows_attn) return bwd_attention_rows(d, f, a, w, g, ab, s);
    return delta_ready ? obte_attn_bwd_delta_ready(&ab, s) : obte_attn_bwd(&ab, s);
}

// c_attn's backward from the whole dqkv (the attention on every position): dh1 = dqkv W_attn and dW_attn = dqkv^T h1 as their own
// launches, or ONE grid: the block's four weight gradients (K = tokens, full K per tile) and, on the CUs those tiles leave idle, dh1 (K = 3C)
int bwd_c_attn(const obte_block_desc* d, const BlockForm& f, const ActLayout& a, const WsLayout& w, const Grads& g, const obte_bf16* dy_mlp,
               const obte_bf16* dx1_proj, obte_stream s) {
    const int C = d->n_embd;
    const obte_gemm_args dh1 = dyW(w.dqkv, d->attn_w, w.dh, f.M, C, 3 * C);
    const obte_gemm_args dw_attn = aTb(w.dqkv, a.h1, g.attn_w, 3 * C, C, f.M);
    if (!f.grouped) {
        TRY(run(dh1, s));
        return run(dw_attn, s, w.gemmws, w.gemmws_bytes);
    }
    const obte_gemm_args gs[5] = {aTb(w.dhpre, a.h2, g.fc_w, 4 * C, C, f.M), aTb(dy_mlp, a.hact, g.mlp_w, C, 4 * C, f.M), dw_attn,
                                  aTb(dx1_proj, a.y, g.proj_w, C, C, f.M), dh1};
    return obte_gemm_grouped_bf16(gs, 5, s);
}

}  // namespace

extern "C" int64_t obte_block_act_bytes(int64_t B, int64_t T, int32_t n_embd, int32_t n_head) { return ActLayout(B, T, n_embd, n_head).total; }
extern "C" int64_t obte_block_act_bytes_p(int64_t B, int64_t T, int32_t n_embd, int32_t n_head, float dropout_p) {
    return ActLayout(B, T, n_embd, n_head, dropout_p > 0.f).total;
}
extern "C" int64_t obte_block_bwd_ws_bytes(int64_t B, int64_t T, int32_t n_embd, int32_t n_head) { return WsLayout(B, T, n_embd, n_head).total; }

extern "C" int obte_block_fwd(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, void* act, obte_stream s) {
    TRY(check_desc("obte_block_fwd", d));
    OBTE_REQUIRE(x && y_out && act, "obte_block_fwd: null pointer");
    const BlockForm f = resolve(d);
    const ActLayout a(d->B, d->T, d->n_embd, d->n_head, true, act);
    TRY(fwd_attention(d, f, a, x, s));
    // the attention projection, x1 = x + dropout(y W_proj^T), and the MLP half: on every position, or (rows form) on the wanted positions only
    const int C = d->n_embd;
    if (f.rows) TRY(fwd_proj_rows(d, f, a, x, s));
    else TRY(run(plus_residual(xWt(a.y, d->proj_w, a.x1, f.M, C, C), x, d->dropout_p, d->dropout_seed, SITE_RESID), s));
    return fwd_mlp(d, f, a, f.rows ? a.rows_x1 : a.x1, y_out, s);
}

// ---- forward without a backward ---------------------------------------------------------------------------------------------------------
// obte_block_fwd's full form, product for product (the same plans, the same dropout masks), with the activation-only c_fc epilogue; no
// keep bits for a backward that will not come.  x is last read by the attention projection's residual add and y_out is written by the
// last product alone, so the two may be one buffer.
extern "C" int64_t obte_block_infer_ws_bytes(int64_t B, int64_t T, int32_t n_embd, int32_t n_head) {
    if (B <= 0 || T <= 0 || n_head <= 0 || n_embd <= 0 || n_embd % n_head != 0 || n_embd % 64 != 0 || n_embd > 4096) return 0;
    const int hs = n_embd / n_head;
    if (hs != 64 && hs != 128) return 0;
    return InferLayout(B, T, n_embd, n_head).total;
}

namespace {

// The one sequence of a forward nobody will differentiate, on M rows laid out in `w`: obte_block_fwd_infer (the attention over the call's
// own positions), obte_block_fwd_prefill (the same, and the rotated keys and the values kept), obte_block_decode (one new position per
// row against the cache), obte_block_extend (n new positions per row against it) and obte_block_decode_shared (one new position per row against
// a prefix cache shared by the row's group and the row's own suffix cache).  rope_cos / rope_sin / rope_T: what c_attn's epilogue rotates by (position = row % rope_T).
struct InferAttention {
    obte_bf16* kv_cache; int64_t T_max;   // the layer's cache (null: obte_block_fwd_infer)
    int64_t pos;                          // against the cache: every row's first new position
    void* dec_ws; int64_t dec_ws_bytes;   // against the cache: the workspace of obte_attn_decode (decode) or obte_attn_extend
    const int32_t* pos_rows = nullptr;    // one position per row: device int32 [B]; pos is then their bound, c_attn stays unrotated and the rotation
                                          // joins the cache store (rope_cos / rope_sin: the FULL tables)
    int64_t n_new = 0;                    // > 0: against the cache, n_new new positions per row; 0: the attention of the call's own T positions
    bool decode = false;                  // n_new == 1 on the one-query launchers (obte_block_decode, obte_block_decode_rows)
    bool kv8 = false;                     // the cache is the e4m3 one (include/omnibiote_hip_kv8.h): prefill and decode only
    const char* who = "";                 // the entry point that the cache's launchers name in an error where they take a name
    // a prefix shared by groups of rows (obte_block_decode_shared, include/omnibiote_hip_shared.h): the prefix cache of P rows holding n_prefix
    // positions; kv_cache / T_max / pos are then the SUFFIX cache of B rows, its slots and the step's slot (decode, uniform)
    const obte_bf16* prefix_cache = nullptr; int64_t P = 0, T_pre = 0, n_prefix = 0;
    // the four weights as codes and scales, in the order of the products below, in the format w_format names: W_E4M3 (obte_block_step_w8,
    // include/omnibiote_hip_w8.h: fp32 row scales) or W_MXFP4 (obte_block_step_w4, include/omnibiote_hip_w4.h: e8m0 block scales); W_BF16: bf16
    // from the descriptor, which holds the dequantised weights either way
    enum WFormat { W_BF16, W_E4M3, W_MXFP4 };
    WFormat w_format = W_BF16; const void* const* w_codes = nullptr; const void* const* w_scales = nullptr;
    // with prefix_cache: suffix slot j of row b is read from the group's row ancestry[b][j] (obte_block_decode_beam, include/omnibiote_hip_beam.h)
    const int32_t* ancestry = nullptr;
    // the cache in pages (include/omnibiote_hip_paged.h): kv_cache is the layer's pool of n_pages pages and page_table [B, table_ld] says where
    // each row's positions lie; prefill, and decode or (bf16) n_new positions per row in the rows form (T_max is not read)
    const int32_t* page_table = nullptr; int64_t n_pages = 0, table_ld = 0;
};
int infer_sequence(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, const InferLayout& w, int64_t M, const float* rope_cos,
                   const float* rope_sin, int64_t rope_T, const InferAttention& at, obte_stream s) {
    const int C = d->n_embd, H = d->n_head, hs = C / H;
    // a call against the cache — decode (M = B rows) or extend (M = B * n_new rows) — of at most obte_small_m_max() rows: its four
    // products on the weight-streaming kernel (gemm_small_m.hip), the same epilogues; every other call (prefill, the forward-only block,
    // a larger extend) on the tile structures at every M.  `which`: the product's place among the four, for the e4m3 form of the streamed weight
    const bool stream_w = at.n_new > 0 && M <= obte_small_m_max();
    auto run = [stream_w, &at](const obte_gemm_args& g, int which, obte_stream st) {
        if (!stream_w) return obte_gemm_bf16_ws(&g, nullptr, 0, st);
        switch (at.w_format) {
            case InferAttention::W_E4M3: return obte_linear_small_m_w8(&g, at.w_codes[which], g.K, (const float*)at.w_scales[which], st);
            case InferAttention::W_MXFP4: return obte_linear_small_m_w4(&g, at.w_codes[which], g.K / 2, at.w_scales[which], g.K / 32, st);
            default: return obte_linear_small_m_bf16(&g, st);
        }
    };
    TRY(obte_layernorm_fwd(x, d->ln1_w, w.h1, w.mean, w.rstd, M, C, 1e-5f, s));
    obte_gemm_args qkv = xWt(w.h1, d->attn_w, w.qkv, M, 3 * C, C);
    if (!at.pos_rows) { qkv.epilogue = OBTE_EPI_ROPE_QK; qkv.rope_cos = rope_cos; qkv.rope_sin = rope_sin; qkv.rope_T = rope_T; qkv.rope_head_dim = hs; }
    TRY(run(qkv, 0, s));
    const float scale = 8.0f / (float)C;  // model.py:119
    if (at.n_new > 0) {   // n_new positions per row join the cache (the rows form rotates them as it stores), then each attends over those up to its own
        const int64_t q_ld = 3 * (int64_t)C;
        const char* who = at.kv8 || at.pos_rows ? at.who : "obte_attn_decode";   // (the uniform bf16 step's attention refuses under its own name)
        if (at.page_table && !at.decode)   // (n_new positions per row through the page table: include/omnibiote_hip_paged_extend.h; bf16, rows form)
            TRY(obte_kv_paged_rope_store_chunk(w.qkv, rope_cos, rope_sin, at.pos_rows, at.pos, d->B, at.n_new, H, hs, at.kv_cache, at.n_pages, at.page_table, at.table_ld, s));
        else if (at.page_table && at.kv8)   // (the rows-form decode step through the page table; the e4m3 pool: include/omnibiote_hip_paged8.h)
            TRY(obte_kv8_paged_rope_store_rows(w.qkv, rope_cos, rope_sin, at.pos_rows, at.pos, d->B, H, hs, at.kv_cache, at.n_pages, at.page_table, at.table_ld, s));
        else if (at.page_table)
            TRY(obte_kv_paged_rope_store_rows(w.qkv, rope_cos, rope_sin, at.pos_rows, at.pos, d->B, H, hs, at.kv_cache, at.n_pages, at.page_table, at.table_ld, s));
        else
            TRY(obte_kv_store_on(at.kv8, at.who, w.qkv, rope_cos, rope_sin, at.pos_rows, at.pos, d->B, at.n_new, H, hs, at.kv_cache, at.T_max, s));
        if (at.page_table && !at.decode)   // row b's n_new queries over its keys up to each one's own position, each key read from its page
            TRY(obte_attn_extend_paged(w.qkv, q_ld, at.kv_cache, at.n_pages, at.page_table, at.table_ld, w.att, nullptr, d->B, at.n_new, at.pos, at.pos_rows, H, hs, scale, 0,
                                       at.dec_ws, at.dec_ws_bytes, s));
        else if (at.page_table)    // row b over its own pos_rows[b] + 1 keys, each read from its page
            TRY(obte_attn_decode_paged_on(at.kv8, who, w.qkv, q_ld, at.kv_cache, at.n_pages, at.page_table, at.table_ld, w.att, nullptr, d->B, at.pos_rows, 1, at.pos + 1, H, hs,
                                          scale, 0, at.dec_ws, at.dec_ws_bytes, s));
        else if (at.prefix_cache && at.ancestry)   // the same, the slots 0 .. pos read through the ancestry table
            TRY(obte_attn_decode_beam(w.qkv, q_ld, at.prefix_cache, at.P, at.T_pre, at.n_prefix, at.kv_cache, d->B / at.P, at.T_max, at.pos + 1, at.ancestry, w.att, nullptr, H,
                                      hs, scale, 0, 0, at.dec_ws, at.dec_ws_bytes, s));
        else if (at.prefix_cache)    // the group's prefix once per 32 rows, then the row's own slots 0 .. pos
            TRY(obte_attn_decode_shared(w.qkv, q_ld, at.prefix_cache, at.P, at.T_pre, at.n_prefix, at.kv_cache, d->B / at.P, at.T_max, at.pos + 1, w.att, nullptr, H, hs,
                                        scale, 0, 0, at.dec_ws, at.dec_ws_bytes, s));
        else if (!at.decode)
            TRY(obte_attn_extend(w.qkv, q_ld, at.kv_cache, w.att, nullptr, d->B, at.T_max, at.n_new, at.pos, at.pos_rows, H, hs, scale, 0, at.dec_ws, at.dec_ws_bytes, s));
        else                    // uniform (pos_rows null: every row over pos + 1 keys) or row b over its own pos_rows[b] + 1
            TRY(obte_attn_decode_on(at.kv8, who, w.qkv, q_ld, at.kv_cache, w.att, nullptr, d->B, at.T_max, at.pos + 1, at.pos_rows, 1, H, hs, scale, 0, at.dec_ws,
                                    at.dec_ws_bytes, s));
    } else {
        obte_attn_fwd_args af = {};
        af.qkv = w.qkv; af.o = w.att; af.lse = w.lse; af.key_ranges = d->key_ranges; af.mask = d->mask;
        af.mask_sb = d->mask_sb; af.mask_sh = d->mask_sh; af.mask_sq = d->mask_sq; af.ranges_exact = d->ranges_exact;
        af.B = d->B; af.T = d->T; af.n_head = H; af.head_dim = hs; af.scale = scale;
        af.dropout_p = d->dropout_p; af.dropout_seed = d->dropout_seed;
        TRY(obte_attn_fwd(&af, s));
        if (at.page_table && at.kv8) TRY(obte_kv8_paged_store(w.qkv, d->B, d->T, H, hs, at.kv_cache, at.n_pages, at.page_table, at.table_ld, s));
        else if (at.page_table) TRY(obte_kv_paged_store(w.qkv, d->B, d->T, H, hs, at.kv_cache, at.n_pages, at.page_table, at.table_ld, s));
        else if (at.kv_cache) TRY(obte_kv_store_on(at.kv8, at.who, w.qkv, nullptr, nullptr, nullptr, 0, d->B, d->T, H, hs, at.kv_cache, at.T_max, s));   // (c_fc's activation overwrites qkv below)
    }
    TRY(run(plus_residual(xWt(w.att, d->proj_w, w.x1, M, C, C), x, d->dropout_p, d->dropout_seed, SITE_RESID), 1, s));
    TRY(obte_layernorm_fwd(w.x1, d->ln2_w, w.h2, w.mean, w.rstd, M, C, 1e-5f, s));
    obte_gemm_args fc = xWt(w.h2, d->fc_w, w.hact, M, 4 * C, C);
    fc.epilogue = OBTE_EPI_GELU_ACT;
    TRY(run(fc, 2, s));
    return run(plus_residual(xWt(w.hact, d->mlp_w, y_out, M, C, 4 * C), w.x1, d->dropout_p, d->dropout_seed, SITE_MLP), 3, s);
}

// obte_block_fwd_infer and obte_block_fwd_prefill: the same checks, the same workspace
int infer_or_prefill(const char* who, const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, void* ws, int64_t ws_bytes, obte_bf16* kv_cache,
                     int64_t T_max, bool prefill, obte_stream s, bool kv8 = false, const int32_t* page_table = nullptr, int64_t n_pages = 0) {   // (paged: T_max is 64 table_ld)
    TRY(check_desc(who, d));
    if (d->out_rows) {
        obte_set_error("%s: the rows form (out_rows) stays with obte_block_fwd", who);
        return OBTE_EUNSUPPORTED;
    }
    OBTE_REQUIRE(x && y_out && ws && (!prefill || kv_cache), "%s: null pointer", who);
    OBTE_REQUIRE(!prefill || d->T <= T_max, page_table ? "%s: %lld positions do not fit the table's %lld" : "%s: %lld positions do not fit T_max = %lld", who,
                 (long long)d->T, (long long)T_max);
    OBTE_REQUIRE(!kv8 || (((uintptr_t)kv_cache & 15) == 0 && ((uintptr_t)page_table & 3) == 0), "%s: cache8 must be 16-byte aligned, a page table 4-byte aligned", who);
    const InferLayout w(d->B, d->T, d->n_embd, d->n_head, ws);
    OBTE_REQUIRE(ws_bytes >= w.total, "%s: workspace of %lld bytes, obte_block_infer_ws_bytes() asks for %lld", who, (long long)ws_bytes, (long long)w.total);
    InferAttention at = {prefill ? kv_cache : nullptr, T_max, -1, nullptr, 0};
    at.kv8 = kv8; at.who = who;
    at.page_table = page_table; at.n_pages = n_pages; at.table_ld = T_max / OBTE_KV_PAGE;
    return infer_sequence(d, x, y_out, w, d->B * d->T, d->rope_cos, d->rope_sin, d->T, at, s);
}

}  // namespace

extern "C" int obte_block_fwd_infer(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, void* ws, int64_t ws_bytes, obte_stream s) {
    return infer_or_prefill("obte_block_fwd_infer", d, x, y_out, ws, ws_bytes, nullptr, 0, false, s);
}

extern "C" int obte_block_fwd_prefill(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, void* ws, int64_t ws_bytes, obte_bf16* kv_cache,
                                      int64_t T_max, obte_stream s) {
    return infer_or_prefill("obte_block_fwd_prefill", d, x, y_out, ws, ws_bytes, kv_cache, T_max, true, s);
}

extern "C" int obte_block_fwd_prefill_kv8(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, void* ws, int64_t ws_bytes, void* cache8, int64_t T_max,
                                          obte_stream s) {
    return infer_or_prefill("obte_block_fwd_prefill_kv8", d, x, y_out, ws, ws_bytes, (obte_bf16*)cache8, T_max, true, s, true);
}

// into the pages of a pool (include/omnibiote_hip_paged.h)
extern "C" int obte_block_fwd_prefill_paged(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, void* ws, int64_t ws_bytes, obte_bf16* pool, int64_t n_pages,
                                            const int32_t* table, int64_t table_ld, obte_stream s) {
    const char* who = "obte_block_fwd_prefill_paged";
    OBTE_REQUIRE(pool && table, "%s: null pointer", who);
    OBTE_REQUIRE(n_pages > 0 && table_ld > 0 && table_ld < (1ll << 18), "%s: bad shape (n_pages and table_ld at least 1)", who);
    return infer_or_prefill(who, d, x, y_out, ws, ws_bytes, pool, OBTE_KV_PAGE * table_ld, true, s, false, table, n_pages);
}

// into the pages of an e4m3 pool (include/omnibiote_hip_paged8.h): both flags of InferAttention
extern "C" int obte_block_fwd_prefill_paged8(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, void* ws, int64_t ws_bytes, void* pool8, int64_t n_pages,
                                             const int32_t* table, int64_t table_ld, obte_stream s) {
    const char* who = "obte_block_fwd_prefill_paged8";
    OBTE_REQUIRE(pool8 && table, "%s: null pointer", who);
    OBTE_REQUIRE(n_pages > 0 && n_pages < (1ll << 24) && table_ld > 0 && table_ld < (1ll << 18), "%s: bad shape (n_pages in [1, 2^24), table_ld at least 1)", who);
    return infer_or_prefill(who, d, x, y_out, ws, ws_bytes, (obte_bf16*)pool8, OBTE_KV_PAGE * table_ld, true, s, true, table, n_pages);
}

// ---- new positions per row against the cache --------------------------------------------------------------------------------------------
namespace {

// obte_block_decode, obte_block_decode_rows and obte_block_extend: d->T new positions per row, every row's from `pos` on or (rows) row b's from
// pos_rows[b] on, read on the device, with `pos` the host's bound on it.  decode: the one-position launchers (obte_kv_cache_rope_store_rows,
// obte_attn_decode / _rows and their workspace behind InferLayout) instead of obte_attn_extend's.
int cached_step(const char* who, const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, obte_bf16* kv_cache, int64_t T_max, int64_t pos,
                const int32_t* pos_rows, bool rows, bool decode, void* ws, int64_t ws_bytes, obte_stream s, bool kv8 = false,
                InferAttention::WFormat w_format = InferAttention::W_BF16, const void* const* w_codes = nullptr, const void* const* w_scales = nullptr, const int32_t* page_table = nullptr, int64_t n_pages = 0) {   // (paged: T_max is 64 table_ld)
    TRY(check_desc(who, d));
    OBTE_REQUIRE(!decode || d->T == 1, "%s: one new position per row (T = 1), got T = %lld", who, (long long)d->T);
    if (d->key_ranges || d->mask || d->query_bounds || d->out_rows || d->dropout_p > 0.f) {
        obte_set_error("%s: key_ranges, mask, query_bounds, out_rows and dropout_p must be NULL / 0 (a new position sees every cached one up to itself)", who);
        return OBTE_EUNSUPPORTED;
    }
    OBTE_REQUIRE(x && y_out && kv_cache && ws && (!rows || pos_rows), "%s: null pointer", who);
    const int64_t n = d->T;
    if (!(pos >= 0 && pos + n <= T_max)) {   // one condition, said in each caller's terms
        if (!decode)
            obte_set_error("%s: positions [%lld, %lld) (d->T = %lld new ones) do not fit the cache's [0, %lld)", who, (long long)pos, (long long)(pos + n),
                           (long long)n, (long long)T_max);
        else
            obte_set_error(rows ? "%s: max_pos = %lld outside the cache's [0, %lld)" : "%s: position %lld outside the cache's [0, %lld)", who, (long long)pos,
                           (long long)T_max);
        return OBTE_EINVAL;
    }
    const int C = d->n_embd, H = d->n_head, hs = C / H;
    if (kv8)   // what its two launchers would refuse, before the first launch of the sequence
        OBTE_REQUIRE(((uintptr_t)kv_cache & 15) == 0 && (((uintptr_t)pos_rows | (uintptr_t)page_table) & 3) == 0 && d->B * H <= 65535,
                     "%s: cache8 must be 16-byte aligned, pos_rows and a page table 4-byte aligned, B * n_head <= 65535", who);
    const int64_t att_bytes = decode ? obte_attn_decode_ws_bytes(d->B, H, hs) : obte_attn_extend_ws_bytes(d->B, H, hs, n, 0);
    OBTE_REQUIRE(decode || att_bytes > 0, "%s: bad shape (B * n_head <= 65535)", who);
    const InferLayout w(d->B, n, C, H, ws);
    const int64_t need = w.total + align256(att_bytes);
    OBTE_REQUIRE(ws_bytes >= need, "%s: workspace of %lld bytes, obte_block_%s_ws_bytes() asks for %lld", who, (long long)ws_bytes, decode ? "decode" : "extend",
                 (long long)need);
    InferAttention at = {kv_cache, T_max, pos, (char*)ws + w.total, att_bytes, rows ? pos_rows : nullptr, n, decode, kv8, who};
    at.w_format = w_format; at.w_codes = w_codes; at.w_scales = w_scales;
    at.page_table = page_table; at.n_pages = n_pages; at.table_ld = T_max / OBTE_KV_PAGE;
    // uniform: c_attn rotates row b n + j by the tables' row pos + j (rope_T = n on the tables advanced by pos rows); rows form: the FULL tables
    const int64_t row = at.pos_rows ? 0 : pos * (hs / 2);
    return infer_sequence(d, x, y_out, w, d->B * n, d->rope_cos + row, d->rope_sin + row, n, at, s);
}

}  // namespace

// InferLayout at T = 1 (M = B rows) with obte_attn_decode's partials behind it
extern "C" int64_t obte_block_decode_ws_bytes(int64_t B, int32_t n_embd, int32_t n_head) {
    const int64_t base = obte_block_infer_ws_bytes(B, 1, n_embd, n_head);
    return base > 0 ? base + align256(obte_attn_decode_ws_bytes(B, n_head, n_embd / n_head)) : 0;
}

extern "C" int obte_block_decode(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, obte_bf16* kv_cache, int64_t T_max, int64_t pos, void* ws,
                                 int64_t ws_bytes, obte_stream s) {
    return cached_step("obte_block_decode", d, x, y_out, kv_cache, T_max, pos, nullptr, false, true, ws, ws_bytes, s);
}

extern "C" int obte_block_decode_rows(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, obte_bf16* kv_cache, int64_t T_max, const int32_t* pos,
                                      int64_t max_pos, void* ws, int64_t ws_bytes, obte_stream s) {
    return cached_step("obte_block_decode_rows", d, x, y_out, kv_cache, T_max, max_pos, pos, true, true, ws, ws_bytes, s);
}

// the rows form on the pages of a pool (include/omnibiote_hip_paged.h)
extern "C" int obte_block_decode_paged(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, obte_bf16* pool, int64_t n_pages, const int32_t* table,
                                       int64_t table_ld, const int32_t* pos, int64_t max_pos, void* ws, int64_t ws_bytes, obte_stream s) {
    const char* who = "obte_block_decode_paged";
    OBTE_REQUIRE(pool && table, "%s: null pointer", who);
    OBTE_REQUIRE(n_pages > 0 && table_ld > 0 && table_ld < (1ll << 18), "%s: bad shape (n_pages and table_ld at least 1)", who);
    return cached_step(who, d, x, y_out, pool, OBTE_KV_PAGE * table_ld, max_pos, pos, true, true, ws, ws_bytes, s, false, InferAttention::W_BF16, nullptr, nullptr, table, n_pages);
}

// the same on the pages of an e4m3 pool (include/omnibiote_hip_paged8.h)
extern "C" int obte_block_decode_paged8(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, void* pool8, int64_t n_pages, const int32_t* table,
                                        int64_t table_ld, const int32_t* pos, int64_t max_pos, void* ws, int64_t ws_bytes, obte_stream s) {
    const char* who = "obte_block_decode_paged8";
    OBTE_REQUIRE(pool8 && table, "%s: null pointer", who);
    OBTE_REQUIRE(n_pages > 0 && n_pages < (1ll << 24) && table_ld > 0 && table_ld < (1ll << 18), "%s: bad shape (n_pages in [1, 2^24), table_ld at least 1)", who);
    return cached_step(who, d, x, y_out, (obte_bf16*)pool8, OBTE_KV_PAGE * table_ld, max_pos, pos, true, true, ws, ws_bytes, s, true, InferAttention::W_BF16, nullptr, nullptr, table, n_pages);
}

// the two on the e4m3 cache (include/omnibiote_hip_kv8.h): pos_rows null or not
extern "C" int obte_block_decode_kv8(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, void* cache8, int64_t T_max, int64_t pos, const int32_t* pos_rows,
                                     void* ws, int64_t ws_bytes, obte_stream s) {
    return cached_step("obte_block_decode_kv8", d, x, y_out, (obte_bf16*)cache8, T_max, pos, pos_rows, pos_rows != nullptr, true, ws, ws_bytes, s, true);
}

// the decode step with its four products' weights in e4m3 (include/omnibiote_hip_w8.h): any of the three above by (cache_e4m3, pos_rows)
extern "C" int obte_block_step_w8(const obte_block_desc* d, const void* const* codes, const float* const* scales, const obte_bf16* x, obte_bf16* y_out, void* cache,
                                  int32_t cache_e4m3, int64_t T_max, int64_t pos, const int32_t* pos_rows, void* ws, int64_t ws_bytes, obte_stream s) {
    const char* who = "obte_block_step_w8";
    OBTE_REQUIRE(codes && scales, "%s: null pointer", who);
    for (int i = 0; i < 4; ++i) {
        OBTE_REQUIRE(codes[i] && scales[i], "%s: null pointer (codes[%d] / scales[%d])", who, i, i);
        OBTE_REQUIRE(((uintptr_t)codes[i] & 15) == 0 && ((uintptr_t)scales[i] & 3) == 0, "%s: codes[%d] must be 16-byte aligned, scales[%d] 4-byte aligned", who, i, i);
    }
    return cached_step(who, d, x, y_out, (obte_bf16*)cache, T_max, pos, pos_rows, pos_rows != nullptr, true, ws, ws_bytes, s, cache_e4m3 != 0, InferAttention::W_E4M3, codes,
                       (const void* const*)scales);
}

// the same with the weights in MXFP4 (include/omnibiote_hip_w4.h)
extern "C" int obte_block_step_w4(const obte_block_desc* d, const void* const* codes, const void* const* scales, const obte_bf16* x, obte_bf16* y_out, void* cache,
                                  int32_t cache_e4m3, int64_t T_max, int64_t pos, const int32_t* pos_rows, void* ws, int64_t ws_bytes, obte_stream s) {
    const char* who = "obte_block_step_w4";
    OBTE_REQUIRE(codes && scales, "%s: null pointer", who);
    for (int i = 0; i < 4; ++i) {
        OBTE_REQUIRE(codes[i] && scales[i], "%s: null pointer (codes[%d] / scales[%d])", who, i, i);
        OBTE_REQUIRE(((uintptr_t)codes[i] & 7) == 0 && ((uintptr_t)scales[i] & 1) == 0, "%s: codes[%d] must be 8-byte aligned, scales[%d] 2-byte aligned", who, i, i);
    }
    return cached_step(who, d, x, y_out, (obte_bf16*)cache, T_max, pos, pos_rows, pos_rows != nullptr, true, ws, ws_bytes, s, cache_e4m3 != 0, InferAttention::W_MXFP4, codes,
                       scales);
}

// InferLayout at T = n_new (M = B n_new rows) with obte_attn_extend's partials behind it (include/omnibiote_hip_extend.h)
extern "C" int64_t obte_block_extend_ws_bytes(int64_t B, int64_t n_new, int32_t n_embd, int32_t n_head) {
    const int64_t base = obte_block_infer_ws_bytes(B, n_new, n_embd, n_head);
    const int64_t part = base > 0 ? obte_attn_extend_ws_bytes(B, n_head, n_embd / n_head, n_new, 0) : 0;
    return part > 0 ? base + align256(part) : 0;
}

extern "C" int obte_block_extend(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, obte_bf16* kv_cache, int64_t T_max, int64_t pos,
                                 const int32_t* pos_rows, void* ws, int64_t ws_bytes, obte_stream s) {
    return cached_step("obte_block_extend", d, x, y_out, kv_cache, T_max, pos, pos_rows, pos_rows != nullptr, false, ws, ws_bytes, s);
}

// the rows form on the pages of a pool (include/omnibiote_hip_paged_extend.h)
extern "C" int obte_block_extend_paged(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, obte_bf16* pool, int64_t n_pages, const int32_t* table,
                                       int64_t table_ld, int64_t pos, const int32_t* pos_rows, void* ws, int64_t ws_bytes, obte_stream s) {
    const char* who = "obte_block_extend_paged";
    OBTE_REQUIRE(pool && table && pos_rows, "%s: null pointer", who);
    OBTE_REQUIRE(n_pages > 0 && n_pages < (1ll << 24) && table_ld > 0 && table_ld < (1ll << 18), "%s: bad shape (n_pages in [1, 2^24), table_ld at least 1)", who);
    OBTE_REQUIRE(((uintptr_t)pool & 15) == 0 && (((uintptr_t)pos_rows | (uintptr_t)table) & 3) == 0, "%s: pool must be 16-byte aligned, pos_rows and table 4-byte aligned",
                 who);
    return cached_step(who, d, x, y_out, pool, OBTE_KV_PAGE * table_ld, pos, pos_rows, true, false, ws, ws_bytes, s, false, InferAttention::W_BF16, nullptr, nullptr, table,
                       n_pages);
}

// InferLayout at T = 1 (M = P G rows) with obte_attn_decode_shared's partials behind it (include/omnibiote_hip_shared.h)
extern "C" int64_t obte_block_decode_shared_ws_bytes(int64_t P, int64_t G, int32_t n_embd, int32_t n_head) {
    if (P <= 0 || G <= 0 || P > 65535 || G >= (1ll << 20)) return 0;
    const int64_t base = obte_block_infer_ws_bytes(P * G, 1, n_embd, n_head);
    const int64_t part = base > 0 ? obte_attn_decode_shared_ws_bytes(P, G, n_head, n_embd / n_head, 0, 0) : 0;
    return part > 0 ? base + align256(part) : 0;
}

namespace {

// obte_block_decode's sequence with the cache in two parts: the new position joins the row's suffix cache at slot suf_pos, and is rotated
// as absolute position n_prefix + suf_pos.  beam (obte_block_decode_beam): the suffix slots are read through `ancestry`
int decode_shared_step(const char* who, bool beam, const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, const obte_bf16* prefix_cache, int64_t P, int64_t T_pre,
                       int64_t n_prefix, obte_bf16* suffix_cache, int64_t T_suf, int64_t suf_pos, const int32_t* ancestry, void* ws, int64_t ws_bytes, obte_stream s) {
    TRY(check_desc(who, d));
    OBTE_REQUIRE(d->T == 1, "%s: one new position per row (T = 1), got T = %lld", who, (long long)d->T);
    if (d->key_ranges || d->mask || d->query_bounds || d->out_rows || d->dropout_p > 0.f) {
        obte_set_error("%s: key_ranges, mask, query_bounds, out_rows and dropout_p must be NULL / 0 (a new position sees every cached one up to itself)", who);
        return OBTE_EUNSUPPORTED;
    }
    OBTE_REQUIRE(x && y_out && prefix_cache && suffix_cache && ws && (!beam || ancestry), "%s: null pointer", who);
    OBTE_REQUIRE(P >= 1 && d->B % P == 0, "%s: the %lld rows are not P = %lld groups of equal size", who, (long long)d->B, (long long)P);
    OBTE_REQUIRE(T_pre >= 1 && n_prefix >= 1 && n_prefix <= T_pre, "%s: n_prefix = %lld outside [1, T_pre = %lld]", who, (long long)n_prefix, (long long)T_pre);
    OBTE_REQUIRE(suf_pos >= 0 && suf_pos < T_suf, "%s: suffix slot %lld outside the suffix cache's [0, %lld)", who, (long long)suf_pos, (long long)T_suf);
    OBTE_REQUIRE((((uintptr_t)prefix_cache | (uintptr_t)suffix_cache) & 15) == 0, "%s: both caches must be 16-byte aligned", who);
    OBTE_REQUIRE(((uintptr_t)ancestry & 3) == 0, "%s: ancestry must be 4-byte aligned", who);
    const int C = d->n_embd, H = d->n_head, hs = C / H;
    const int64_t G = d->B / P;
    const int64_t att_bytes = obte_attn_decode_shared_ws_bytes(P, G, H, hs, 0, 0);
    OBTE_REQUIRE(att_bytes > 0 && T_pre < (1ll << 24) && T_suf < (1ll << 24), "%s: bad shape (P * n_head and B * n_head <= 65535)", who);
    const InferLayout w(d->B, 1, C, H, ws);
    const int64_t need = w.total + align256(att_bytes);
    OBTE_REQUIRE(ws_bytes >= need, "%s: workspace of %lld bytes, %s_ws_bytes() asks for %lld", who, (long long)ws_bytes, who, (long long)need);
    InferAttention at = {suffix_cache, T_suf, suf_pos, (char*)ws + w.total, att_bytes, nullptr, 1, true, false, who};
    at.prefix_cache = prefix_cache; at.P = P; at.T_pre = T_pre; at.n_prefix = n_prefix; at.ancestry = beam ? ancestry : nullptr;
    const int64_t row = (n_prefix + suf_pos) * (hs / 2);   // c_attn rotates every row by the tables' row n_prefix + suf_pos (rope_T = 1)
    return infer_sequence(d, x, y_out, w, d->B, d->rope_cos + row, d->rope_sin + row, 1, at, s);
}

}  // namespace

extern "C" int obte_block_decode_shared(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, const obte_bf16* prefix_cache, int64_t P, int64_t T_pre,
                                        int64_t n_prefix, obte_bf16* suffix_cache, int64_t T_suf, int64_t suf_pos, void* ws, int64_t ws_bytes, obte_stream s) {
    return decode_shared_step("obte_block_decode_shared", false, d, x, y_out, prefix_cache, P, T_pre, n_prefix, suffix_cache, T_suf, suf_pos, nullptr, ws, ws_bytes, s);
}

// the same step with the suffix slots read through an ancestry table (include/omnibiote_hip_beam.h): the same workspace
extern "C" int64_t obte_block_decode_beam_ws_bytes(int64_t P, int64_t G, int32_t n_embd, int32_t n_head) { return obte_block_decode_shared_ws_bytes(P, G, n_embd, n_head); }

extern "C" int obte_block_decode_beam(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y_out, const obte_bf16* prefix_cache, int64_t P, int64_t T_pre,
                                      int64_t n_prefix, obte_bf16* suffix_cache, int64_t T_suf, int64_t suf_pos, const int32_t* ancestry, void* ws, int64_t ws_bytes,
                                      obte_stream s) {
    return decode_shared_step("obte_block_decode_beam", true, d, x, y_out, prefix_cache, P, T_pre, n_prefix, suffix_cache, T_suf, suf_pos, ancestry, ws, ws_bytes, s);
}

extern "C" int obte_block_bwd_acc(const obte_block_desc* d, const obte_bf16* x, const obte_bf16* dy, const void* act, void* ws,
                                  obte_bf16* dx, obte_bf16* dln1_w, obte_bf16* dattn_w, obte_bf16* dproj_w, obte_bf16* dln2_w,
                                  obte_bf16* dfc_w, obte_bf16* dmlp_w, int accumulate_matrices, obte_stream s) {
    TRY(check_desc("obte_block_bwd", d));
    const bool mats_unwritten = d->w_acc32_mode == OBTE_ACC32_FIRST || d->w_acc32_mode == OBTE_ACC32_MORE;   // (the fp32 sums take them: may be null)
    OBTE_REQUIRE(x && dy && act && ws && dx && dln1_w && dln2_w && (mats_unwritten || (dattn_w && dproj_w && dfc_w && dmlp_w)), "obte_block_bwd: null pointer");
    const int lnp = d->ln_partial_mode;
    OBTE_REQUIRE(!lnp || (d->ln1_partials && d->ln2_partials && lnp >= OBTE_LN_PARTIAL_FIRST && lnp <= OBTE_LN_PARTIAL_LAST),
                 "obte_block_bwd: ln_partial_mode needs both partial buffers and a valid mode");
    const int wm = d->w_acc32_mode;
    OBTE_REQUIRE(!wm || (d->attn_w_acc32 && d->proj_w_acc32 && d->fc_w_acc32 && d->mlp_w_acc32 && wm >= OBTE_ACC32_FIRST && wm <= OBTE_ACC32_LAST &&
                         !(accumulate_matrices & 1)),
                 "obte_block_bwd: w_acc32_mode needs the four fp32 buffers, a valid mode and accumulate_matrices bit 0 clear");
    // accumulate_matrices: bit 0 = the four matrices, bit 1 = the two LayerNorm weights
    const bool acc = (accumulate_matrices & 1) != 0;
    const Grads g = {dln1_w, dln2_w, Wgrad{dattn_w, acc, d->attn_w_acc32, wm}, Wgrad{dproj_w, acc, d->proj_w_acc32, wm},
                     Wgrad{dfc_w, acc, d->fc_w_acc32, wm}, Wgrad{dmlp_w, acc, d->mlp_w_acc32, wm}, (accumulate_matrices & 2) ? 1 : 0};
    const BlockForm f = resolve(d);
    const ActLayout a(d->B, d->T, d->n_embd, d->n_head, true, act);   // (only read here)
    const WsLayout w(d->B, d->T, d->n_embd, d->n_head, ws);
    const obte_bf16 *dy_mlp = nullptr, *dx1_proj = nullptr;   // the two incoming gradients as their projections see them (under the dropout masks)
    bool delta_ready = false;   // what obte_gemm_rowdot_bf16 answered: a run-time result, not part of the form
    TRY(bwd_mlp(d, f, a, w, g, dy, &dy_mlp, s));
    TRY(f.rows ? bwd_ln2_proj_rows(d, f, a, w, g, dy, s) : bwd_ln2_proj_full(d, f, a, w, g, dy, &dx1_proj, &delta_ready, s));
    TRY(bwd_attention(d, f, a, w, g, delta_ready, s));
    if (!f.rows_attn) TRY(bwd_c_attn(d, f, a, w, g, dy_mlp, dx1_proj, s));
    // dx = dx1 + LN1'(dh1); with dropout and a block below, also dropout(dx) under that block's (seed, site 3) mask
    return ln_bwd(d, g, w, w.dh, x, d->ln1_w, a.mean1, a.rstd1, w.dx1, dx, g.ln1_w, d->ln1_partials, f.M, s,
                  f.drop ? d->dx_masked : nullptr, d->dx_mask_seed, SITE_MLP);
}

extern "C" int obte_block_bwd(const obte_block_desc* d, const obte_bf16* x, const obte_bf16* dy, const void* act, void* ws,
                              obte_bf16* dx, obte_bf16* dln1_w, obte_bf16* dattn_w, obte_bf16* dproj_w, obte_bf16* dln2_w,
                              obte_bf16* dfc_w, obte_bf16* dmlp_w, obte_stream s) {
    return obte_block_bwd_acc(d, x, dy, act, ws, dx, dln1_w, dattn_w, dproj_w, dln2_w, dfc_w, dmlp_w, 0, s);
}
