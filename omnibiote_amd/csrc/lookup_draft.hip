// Speculative decoding without a draft model (include/omnibiote_hip_lookup.h): the n-gram lookup that drafts k tokens from a row's own
// history, one launch, one workgroup of 256 threads per row.
//   stage    the row's first n tokens into LDS as 32-bit words, everything outside [0, V) as one sentinel that no comparison accepts
//            (8192 words = 32 KiB: five workgroups per CU).
//   match    thread t walks the candidate ends e = t + 1, t + 257, ... and compares backwards against the row's last tokens, at most
//            g_max steps: the lanes of a wave read consecutive words (no bank conflict), the suffix word is a broadcast.
//   reduce   m << 16 | e (m <= 16, e < 8192) as one u32 maximum: the longest match and, among equals, the most recent end.
//   draft    lane j < k copies hist[e* + (j mod d)], d = n - e*, from global memory: the 64-bit value as it stands, sentinel or not.
// No atomics anywhere; nothing is written but the row's k drafted tokens and its match length.
#include "common.h"
#include "../../include/omnibiote_hip_lookup.h"

namespace {

constexpr int LK_NT = 256;
constexpr int LK_MAX_K = 31;
constexpr uint32_t LK_NONE = 0xFFFFFFFFu;   // a token outside [0, V): V <= 65536, so no token's word is this one

struct LookupParams {
    const int64_t* hist;
    int64_t hist_ld;
    const int32_t* lens;
    int64_t* draft;
    int32_t* match_len;
    int32_t k, g_min, g_max, V;
};

__global__ __launch_bounds__(LK_NT) void lookup_draft_kernel(LookupParams a) {
    __shared__ uint32_t h[OBTE_LOOKUP_MAX_HISTORY];
    __shared__ uint32_t red[LK_NT / 64];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t len = (int64_t)a.lens[b];
    int64_t* draft = a.draft + b * a.k;
    if (len < 1 || len > a.hist_ld) {   // (uniform over the workgroup) an inactive row: its history is not read
        if (tid < a.k) draft[tid] = 0;
        if (tid == 0) a.match_len[b] = 0;
        return;
    }
    const int n = (int)len;             // 1 <= n <= hist_ld <= 8192
    const int64_t* row = a.hist + b * a.hist_ld;
    for (int i = tid; i < n; i += LK_NT) {
        const int64_t t = row[i];
        h[i] = (uint64_t)t < (uint64_t)a.V ? (uint32_t)t : LK_NONE;
    }
    __syncthreads();
    uint32_t best = 0;
    for (int e = tid + 1; e < n; e += LK_NT) {
        const int lim = min(a.g_max, e);
        int m = 0;
        while (m < lim) {
            const uint32_t x = h[e - 1 - m];
            if (x != h[n - 1 - m] || x == LK_NONE) break;
            ++m;
        }
        best = max(best, ((uint32_t)m << 16) | (uint32_t)e);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < LK_NT / 64; ++w) best = max(best, red[w]);
    int m = (int)(best >> 16), e = (int)(best & 0xFFFFu);
    if (m < a.g_min) { m = 0; e = n - 1; }   // (n = 1: best = 0 and e = 0)
    const int d = n - e;                      // 1 <= d <= n
    if (tid < a.k) draft[tid] = row[e + tid % d];
    if (tid == 0) a.match_len[b] = m;
}

}  // namespace

extern "C" int obte_lookup_draft(const int64_t* hist, int64_t hist_ld, const int32_t* lens, int64_t B, int32_t k, int32_t g_min, int32_t g_max, int64_t V,
                                 int64_t* draft, int32_t* match_len, obte_stream s) {
    const char* who = "obte_lookup_draft";
    OBTE_REQUIRE(hist && lens && draft && match_len, "%s: null pointer (hist, lens, draft, match_len)", who);
    OBTE_REQUIRE(B >= 1 && B < (1ll << 24) && hist_ld >= 1 && k >= 1, "%s: B, hist_ld and k must be at least 1 (B=%lld hist_ld=%lld k=%d)", who, (long long)B,
                 (long long)hist_ld, (int)k);
    if (hist_ld > OBTE_LOOKUP_MAX_HISTORY) {
        obte_set_error("%s: hist_ld = %lld exceeds the %d tokens of a row a workgroup holds in LDS", who, (long long)hist_ld, OBTE_LOOKUP_MAX_HISTORY);
        return OBTE_EUNSUPPORTED;
    }
    if (k > LK_MAX_K) {
        obte_set_error("%s: k = %d exceeds %d drafted tokens (the verification's limit)", who, (int)k, LK_MAX_K);
        return OBTE_EUNSUPPORTED;
    }
    OBTE_REQUIRE(g_min >= 1 && g_min <= g_max && g_max <= OBTE_LOOKUP_MAX_NGRAM, "%s: 1 <= g_min <= g_max <= %d does not hold (g_min=%d g_max=%d)", who,
                 OBTE_LOOKUP_MAX_NGRAM, (int)g_min, (int)g_max);
    OBTE_REQUIRE(V >= 1 && V <= 65536, "%s: V must lie in [1, 65536], got %lld", who, (long long)V);
    OBTE_REQUIRE_ALIGNED(who, hist, "hist", 8);
    OBTE_REQUIRE_ALIGNED(who, draft, "draft", 8);
    OBTE_REQUIRE_ALIGNED(who, lens, "lens", 4);
    OBTE_REQUIRE_ALIGNED(who, match_len, "match_len", 4);
    LookupParams a;
    a.hist = hist; a.hist_ld = hist_ld; a.lens = lens; a.draft = draft; a.match_len = match_len;
    a.k = k; a.g_min = g_min; a.g_max = g_max; a.V = (int32_t)V;
    hipStream_t st = (hipStream_t)s;
    const int prof = obte_prof_begin(st, 122, B, hist_ld, k);
    hipLaunchKernelGGL(lookup_draft_kernel, dim3((unsigned)B), dim3(LK_NT), 0, st, a);
    obte_prof_end(prof, st);
    OBTE_CHECK_LAUNCH(who);
    return OBTE_OK;
}
