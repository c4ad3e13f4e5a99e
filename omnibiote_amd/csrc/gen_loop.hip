// The generation loop's state on the device (include/omnibiote_hip_loop.h): one launch turns a step's sampled tokens into the next
// step's inputs — the row's position, count, output column, EOS parking, the next uniforms and the next embedding row.  One workgroup
// per row; every lane reads the row's four state words (wave-uniform loads), a barrier separates those reads from lane 0's stores, and
// all lanes then copy the embedding row 16 bytes at a time.
#include "common.h"
#include "../../include/omnibiote_hip_loop.h"

namespace {

struct AdvanceParams {
    const int64_t* sampled;
    int32_t* pos;
    int32_t* count;
    int64_t* out;
    int64_t out_ld;
    int32_t* n_new;
    int64_t* token;
    const bf16* wte;
    int64_t vocab;
    bf16* x;
    const float* us;
    int64_t us_steps;
    float* u;
    int64_t eos, B;
    int32_t cols, commit;
};

__global__ __launch_bounds__(256) void gen_advance_kernel(AdvanceParams a) {
    const int64_t b = blockIdx.x;
    int32_t p = a.pos[b];
    const int32_t s = a.count[b];
    const int64_t t = a.sampled[b];
    int64_t tok = a.token[b];
    __syncthreads();                                                  // every lane has read the row's state: lane 0 may overwrite it
    const bool running = p >= 0;
    if (a.commit && running) p = (int32_t)((uint32_t)p + 1u);
    const bool record = running && s >= 0 && (int64_t)s < a.out_ld;
    if (record) {
        tok = t;
        if (a.eos >= 0 && t == a.eos) p = -1;
    }
    if (threadIdx.x == 0) {
        if (record) {
            a.out[b * a.out_ld + s] = t;
            a.n_new[b] += 1;
            a.token[b] = t;
        }
        a.pos[b] = p;
        a.count[b] = (int32_t)((uint32_t)s + 1u);
        if (a.us) {
            int64_t r = (int64_t)s + 1;
            r = r < 0 ? 0 : (r > a.us_steps - 1 ? a.us_steps - 1 : r);
            a.u[b] = a.us[r * a.B + b];
        }
    }
    const int64_t row = tok < 0 ? 0 : (tok >= a.vocab ? a.vocab - 1 : tok);
    const bf16* src = a.wte + row * a.cols;
    bf16* dst = a.x + b * a.cols;
    for (int c = (int)threadIdx.x * 8; c < a.cols; c += 256 * 8)
        *reinterpret_cast<bf16x8*>(dst + c) = *reinterpret_cast<const bf16x8*>(src + c);
}

}  // namespace

extern "C" int obte_gen_advance(const int64_t* sampled, int32_t* pos, int32_t* count, int64_t* out, int64_t out_ld, int32_t* n_new, int64_t* token,
                                const obte_bf16* wte, int64_t vocab, int32_t cols, obte_bf16* x, const float* us, int64_t us_steps, float* u, int64_t eos,
                                int32_t commit, int64_t B, obte_stream s) {
    static const char* who = "obte_gen_advance";
    OBTE_REQUIRE(sampled && pos && count && out && n_new && token && wte && x, "%s: null pointer (sampled, pos, count, out, n_new, token, wte, x)", who);
    OBTE_REQUIRE(!us || u, "%s: null pointer (u, with us given)", who);
    OBTE_REQUIRE(B >= 1 && B < (1ll << 31), "%s: B must lie in [1, 2^31), got %lld", who, (long long)B);
    OBTE_REQUIRE(vocab >= 1, "%s: vocab must be at least 1, got %lld", who, (long long)vocab);
    OBTE_REQUIRE(out_ld >= 1, "%s: out_ld must be at least 1, got %lld", who, (long long)out_ld);
    OBTE_REQUIRE(cols >= 8 && cols % 8 == 0, "%s: cols must be a positive multiple of 8 (16-byte rows), got %d", who, (int)cols);
    OBTE_REQUIRE(!us || us_steps >= 1, "%s: us_steps must be at least 1, got %lld", who, (long long)us_steps);
    OBTE_REQUIRE_ALIGNED(who, wte, "wte", 16);
    OBTE_REQUIRE_ALIGNED(who, x, "x", 16);
    OBTE_REQUIRE_ALIGNED(who, sampled, "sampled", 8);
    OBTE_REQUIRE_ALIGNED(who, out, "out", 8);
    OBTE_REQUIRE_ALIGNED(who, token, "token", 8);
    OBTE_REQUIRE_ALIGNED(who, pos, "pos", 4);
    OBTE_REQUIRE_ALIGNED(who, count, "count", 4);
    OBTE_REQUIRE_ALIGNED(who, n_new, "n_new", 4);
    OBTE_REQUIRE_ALIGNED(who, us, "us", 4);
    OBTE_REQUIRE_ALIGNED(who, u, "u", 4);
    AdvanceParams a;
    a.sampled = sampled; a.pos = pos; a.count = count; a.out = out; a.out_ld = out_ld; a.n_new = n_new; a.token = token;
    a.wte = (const bf16*)wte; a.vocab = vocab; a.x = (bf16*)x; a.us = us; a.us_steps = us_steps; a.u = us ? u : nullptr;
    a.eos = eos; a.B = B; a.cols = cols; a.commit = commit;
    hipLaunchKernelGGL(gen_advance_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)s, a);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}
