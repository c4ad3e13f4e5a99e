// The integer prelude of an optimizer step, for callers of the C ABI that have no tensor library at hand:
//   obte_key_ranges_from_tokens   token ids -> the per-query [k_start, k_end) of the reference's document mask
//   obte_token_order              token ids -> the stable argsort obte_embedding_bwd* takes as `order`
//   obte_causal_bounds            (a document range mask, or nothing) -> the pair of tables of the causal mask under it
// All results are integers with exactly one right answer; neither kernel lets the arrival order of atomics decide where
// anything lands (the only atomics are the LDS counters of the digit histogram), no workgroup waits on another, and every loop
// has a bound known at launch.
#include "common.h"

// =============================================================================================== key ranges
// One workgroup per row.  The row is walked in chunks of KR_CHUNK positions; position base + 256 j + tid belongs to thread
// tid, so the ballot of (wave, j) is the EOS bit mask of 64 consecutive positions: word 4 j + wave of the chunk's 16.  From the
// words in LDS every position reads the next EOS at or after it (a count-trailing-zeros of its own word, else the first EOS of
// the later words, else the carry from beyond the chunk) and the last EOS before it (the mirror image).  The carry from beyond
// the chunk is found by reading ahead until a chunk has an EOS; a chunk is read ahead at most once and walked once.
// The reference's conditions on the number of EOS before a position need no count: none before <=> there is no last EOS
// before it, exactly one before <=> the last EOS before it is the row's first.
#define KR_THREADS 256
#define KR_PER_THREAD 4
#define KR_CHUNK (KR_THREADS * KR_PER_THREAD)
#define KR_WORDS (KR_CHUNK / 64)

__device__ __forceinline__ int kr_first(uint64_t w) { return __builtin_ctzll(w); }
__device__ __forceinline__ int kr_last(uint64_t w) { return 63 - __builtin_clzll(w); }

// the EOS words of chunk `chunk` of the row -> sw[KR_WORDS]; positions at or beyond T hold no EOS
__device__ __forceinline__ void kr_load_words(const int64_t* __restrict__ row, int T, int chunk, int64_t eos, uint64_t* sw) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint64_t m[KR_PER_THREAD];
#pragma unroll
    for (int j = 0; j < KR_PER_THREAD; ++j) {
        const int pos = chunk * KR_CHUNK + j * KR_THREADS + tid;
        const bool f = pos < T && row[pos] == eos;
        m[j] = __ballot(f);
    }
    __syncthreads();   // every reader of the previous chunk's words is done
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < KR_PER_THREAD; ++j) sw[j * (KR_THREADS / 64) + wave] = m[j];
    }
    __syncthreads();
}

__global__ __launch_bounds__(KR_THREADS) void key_ranges_kernel(const int64_t* __restrict__ ids, int T, int64_t eos, int padding,
                                                                 int64_t group, int32_t* __restrict__ out) {
    __shared__ uint64_t sw[KR_WORDS];
    __shared__ int s_prev[KR_WORDS + 1];   // last EOS in the chunk's words < i (chunk-local position), -1: none
    __shared__ int s_next[KR_WORDS];       // first EOS in the chunk's words > i, -1: none
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t b = blockIdx.x;
    const int64_t* row = ids + b * (int64_t)T;
    int32_t* orow = out + b * (int64_t)T * 2;
    const int nch = (T + KR_CHUNK - 1) / KR_CHUNK;
    const int Tx = padding ? T : T + 1;    // the non-padding mode's appended EOS column sits at position T, implied
    const int BIG = Tx + 1;
    const int beyond = padding ? BIG : T;  // the next EOS of a position with no token EOS at or after it
    const bool quirk = (group > 0 ? b % group : b) >= 1;

    // the row's first two EOS (token EOS only; the implied column is added below)
    int r0 = -1, r1 = -1, loaded = -1;
    for (int c = 0; c < nch && r1 < 0; ++c) {
        kr_load_words(row, T, c, eos, sw);
        loaded = c;
        for (int i = 0; i < KR_WORDS; ++i) {
            uint64_t w = sw[i];
            if (w && r0 < 0) { r0 = c * KR_CHUNK + 64 * i + kr_first(w); w &= w - 1; }
            if (w && r0 >= 0 && r1 < 0) r1 = c * KR_CHUNK + 64 * i + kr_first(w);
        }
    }
    const int c1 = r0 >= 0 ? r0 : beyond;
    const int c2 = r1 >= 0 ? r1 : (r0 >= 0 ? beyond : BIG);
    const bool no_eos = padding && r0 < 0;   // without padding the implied column is an EOS of every row

    int prev_carry = -1;   // last EOS before the chunk
    int ahead = -1;        // first EOS at or after the chunk's end; valid while >= that end
    for (int c = 0; c < nch; ++c) {
        const int base = c * KR_CHUNK;
        if (loaded != c) { kr_load_words(row, T, c, eos, sw); loaded = c; }
        if (tid <= KR_WORDS) {
            int p = -1;
            for (int i = 0; i < tid; ++i) { const uint64_t w = sw[i]; if (w) p = 64 * i + kr_last(w); }
            s_prev[tid] = p;
            if (tid < KR_WORDS) {
                int n = -1;
                for (int i = KR_WORDS - 1; i > tid; --i) { const uint64_t w = sw[i]; if (w) n = 64 * i + kr_first(w); }
                s_next[tid] = n;
            }
        }
        __syncthreads();
        uint64_t word[KR_PER_THREAD];
        int wprev[KR_PER_THREAD], wnext[KR_PER_THREAD];
#pragma unroll
        for (int j = 0; j < KR_PER_THREAD; ++j) {
            const int wi = j * (KR_THREADS / 64) + wave;
            word[j] = sw[wi]; wprev[j] = s_prev[wi]; wnext[j] = s_next[wi];
        }
        const int chunk_last = s_prev[KR_WORDS];
        if (ahead < base + KR_CHUNK) {   // uniform over the workgroup: read ahead for the next EOS beyond this chunk
            ahead = beyond;
            bool found = false;
            for (int la = c + 1; la < nch && !found; ++la) {
                kr_load_words(row, T, la, eos, sw);
                loaded = la;
                for (int i = KR_WORDS - 1; i >= 0; --i) {
                    const uint64_t w = sw[i];
                    if (w) { ahead = la * KR_CHUNK + 64 * i + kr_first(w); found = true; }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < KR_PER_THREAD; ++j) {
            const int pos = base + j * KR_THREADS + tid;
            const uint64_t at_or_after = word[j] >> lane;
            const uint64_t before = word[j] & ((1ull << lane) - 1ull);
            const int nxt = at_or_after ? pos + kr_first(at_or_after) : (wnext[j] >= 0 ? base + wnext[j] : ahead);
            const int prv = before ? pos - lane + kr_last(before) : (wprev[j] >= 0 ? base + wprev[j] : prev_carry);
            int start = prv + 1, end = nxt + 1;
            if (quirk && prv < 0 && c2 < BIG) end = c2 + 1;   // the quirk: before the row's first EOS the block runs to the second
            if (quirk && prv >= 0 && prv == c1) start = 0;    // the quirk: the first EOS does not advance the block start
            if (nxt >= BIG) { start = 0; end = 0; }           // never painted: the PAD tail after the last EOS
            if (no_eos) { start = 0; end = T; }               // rows without any EOS attend everywhere
            if (end > T) end = T;
            if (pos < T) *reinterpret_cast<int2*>(orow + 2 * (int64_t)pos) = make_int2(start, end);
        }
        if (chunk_last >= 0) prev_carry = base + chunk_last;
    }
}

extern "C" int obte_key_ranges_from_tokens(const int64_t* ids, int64_t B, int64_t T, int64_t eos_token, int padding, int64_t group,
                                           int32_t* key_ranges, obte_stream s) {
    OBTE_REQUIRE(ids && key_ranges, "obte_key_ranges_from_tokens: null pointer");
    OBTE_REQUIRE_ALIGNED("obte_key_ranges_from_tokens", ids, "ids", 8);
    OBTE_REQUIRE_ALIGNED("obte_key_ranges_from_tokens", key_ranges, "key_ranges", 8);
    OBTE_REQUIRE(B > 0 && B < (1ll << 31) && T > 0 && T < (1ll << 24), "obte_key_ranges_from_tokens: bad shape (1 <= B < 2^31, 1 <= T < 2^24)");
    OBTE_REQUIRE(group >= 0, "obte_key_ranges_from_tokens: group must be >= 0");
    hipLaunchKernelGGL(key_ranges_kernel, dim3((unsigned)B), dim3(KR_THREADS), 0, (hipStream_t)s, ids, (int)T, eos_token,
                       padding ? 1 : 0, group, key_ranges);
    OBTE_CHECK_LAUNCH("obte_key_ranges_from_tokens");
    return OBTE_OK;
}

// =============================================================================================== token order
// Least-significant-digit radix sort, 8 bits per pass, every segment on its own.  A segment is cut into tiles of TO_TILE
// elements; within a tile wave w owns elements [256 w, 256 w + 256) and takes them 64 at a time, so (tile, wave, round, lane)
// is the element order.  A pass is three launches:
//   hist     per tile, the count of every digit                       -> hist[segment][tile][digit]
//   scan     per segment, exclusive prefix in (digit, tile) order, in place: where a tile's run of a digit starts
//   scatter  per tile: each wave counts its own digits (the lanes of a round that share a digit find each other with eight
//            ballots; the lowest of them adds the group's size to the wave's counter, no atomic), the counters of the earlier
//            waves are summed, and an element lands at run start + earlier waves + earlier rounds + lower lanes of its digit.
// Keys (masked to the bits that are sorted on) and segment-local indices ping-pong through the workspace; the first pass reads
// the ids, the last writes the indices to `order`.
#define TO_THREADS 256
#define TO_WAVES (TO_THREADS / 64)
#define TO_ROUNDS 4
#define TO_TILE (TO_THREADS * TO_ROUNDS)
#define TO_RADIX 256

struct ToShape {
    int64_t seg_len;   // elements per segment
    int64_t ntiles;    // tiles per segment
    int shift;         // bit offset of this pass's digit
    uint32_t keymask;  // the bits the whole sort looks at
};

// element e of the segment: its key, from the ids (first pass) or the previous pass's keys
__device__ __forceinline__ uint32_t to_key(const int64_t* __restrict__ ids, const uint32_t* __restrict__ kin, int64_t at, uint32_t keymask) {
    return ids ? ((uint32_t)ids[at] & keymask) : kin[at];
}

__global__ __launch_bounds__(TO_THREADS) void token_hist_kernel(const int64_t* __restrict__ ids, const uint32_t* __restrict__ kin,
                                                                 uint32_t* __restrict__ hist, ToShape sh) {
    __shared__ uint32_t cnt[TO_RADIX];
    const int tid = threadIdx.x;
    const int64_t seg = blockIdx.x / sh.ntiles, tile = blockIdx.x % sh.ntiles;
    cnt[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TO_ROUNDS; ++r) {
        const int64_t e = tile * TO_TILE + r * TO_THREADS + tid;
        if (e < sh.seg_len) atomicAdd(&cnt[(to_key(ids, kin, seg * sh.seg_len + e, sh.keymask) >> sh.shift) & (TO_RADIX - 1)], 1u);
    }
    __syncthreads();
    hist[(int64_t)blockIdx.x * TO_RADIX + tid] = cnt[tid];
}

// one workgroup per segment, thread d owns digit d
__global__ __launch_bounds__(TO_RADIX) void token_scan_kernel(uint32_t* __restrict__ hist, int64_t ntiles) {
    __shared__ uint32_t wsum[TO_RADIX / 64];
    const int d = threadIdx.x, wave = d >> 6, lane = d & 63;
    uint32_t* h = hist + (int64_t)blockIdx.x * ntiles * TO_RADIX + d;
    uint32_t total = 0;
#pragma unroll 8
    for (int64_t t = 0; t < ntiles; ++t) total += h[t * TO_RADIX];
    // exclusive prefix of the digit totals over the 256 digits
    uint32_t inc = total;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t run = inc - total;
    for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll 8
    for (int64_t t = 0; t < ntiles; ++t) {
        const uint32_t c = h[t * TO_RADIX];
        h[t * TO_RADIX] = run;
        run += c;
    }
}

__global__ __launch_bounds__(TO_THREADS) void token_scatter_kernel(const int64_t* __restrict__ ids, const uint32_t* __restrict__ kin,
                                                                    const int32_t* __restrict__ iin, const uint32_t* __restrict__ hist,
                                                                    uint32_t* __restrict__ kout, int32_t* __restrict__ iout, ToShape sh) {
    __shared__ uint32_t cnt[TO_WAVES][TO_RADIX];   // per wave: digit counts, then the running start of the wave's next round
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t seg = blockIdx.x / sh.ntiles, tile = blockIdx.x % sh.ntiles;
    const int64_t segbase = seg * sh.seg_len;
    uint32_t key[TO_ROUNDS], rank[TO_ROUNDS], size[TO_ROUNDS];
    int32_t idx[TO_ROUNDS];
    bool valid[TO_ROUNDS];
#pragma unroll
    for (int w = 0; w < TO_WAVES; ++w) cnt[w][tid] = 0;
#pragma unroll
    for (int r = 0; r < TO_ROUNDS; ++r) {
        const int64_t e = tile * TO_TILE + (int64_t)wave * (64 * TO_ROUNDS) + r * 64 + lane;
        valid[r] = e < sh.seg_len;
        key[r] = valid[r] ? to_key(ids, kin, segbase + e, sh.keymask) : 0u;
        idx[r] = valid[r] ? (iin ? iin[segbase + e] : (int32_t)e) : 0;
        const uint32_t dg = (key[r] >> sh.shift) & (TO_RADIX - 1);
        uint64_t peers = __ballot(valid[r]);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (dg >> bit) & 1u;
            const uint64_t m = __ballot(one);
            peers &= one ? m : ~m;
        }
        rank[r] = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        size[r] = (uint32_t)__popcll(peers);
    }
    __syncthreads();
    // the wave's digit counts: one lane per digit and round adds, rounds in turn (a barrier between them orders the updates)
#pragma unroll
    for (int r = 0; r < TO_ROUNDS; ++r) {
        const uint32_t dg = (key[r] >> sh.shift) & (TO_RADIX - 1);
        if (valid[r] && rank[r] == 0) cnt[wave][dg] += size[r];
        __syncthreads();
    }
    {   // thread d: counts of digit d over the waves -> where each wave's run of d starts in the segment
        uint32_t run = hist[(int64_t)blockIdx.x * TO_RADIX + tid];
#pragma unroll
        for (int w = 0; w < TO_WAVES; ++w) {
            const uint32_t c = cnt[w][tid];
            cnt[w][tid] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TO_ROUNDS; ++r) {
        const uint32_t dg = (key[r] >> sh.shift) & (TO_RADIX - 1);
        const uint32_t start = cnt[wave][dg];
        __syncthreads();
        if (valid[r]) {
            const int64_t off = (int64_t)start + rank[r];   // < seg_len: the counts of a segment sum to seg_len
            if (off < sh.seg_len) {
                if (kout) kout[segbase + off] = key[r];
                iout[segbase + off] = idx[r];
            }
            if (rank[r] == 0) cnt[wave][dg] = start + size[r];
        }
        __syncthreads();
    }
}

static int to_passes(int64_t vocab) {
    int bits = 0;
    while ((1ll << bits) < vocab) ++bits;
    const int p = (bits + 7) / 8;
    return p < 1 ? 1 : p;
}
static bool to_shape_ok(int64_t segments, int64_t seg_len, int64_t vocab) {
    return segments > 0 && seg_len > 0 && vocab >= 1 && vocab <= (1ll << 17) && segments <= ((1ll << 31) - 1) / seg_len;
}
static int64_t to_align(int64_t bytes) { return (bytes + 255) / 256 * 256; }

extern "C" int64_t obte_token_order_ws_bytes(int64_t segments, int64_t seg_len, int64_t vocab) {
    if (!to_shape_ok(segments, seg_len, vocab)) return 0;
    const int64_t n = segments * seg_len, ntiles = cdiv64(seg_len, TO_TILE);
    const int pairs = to_passes(vocab) - 1;   // key + index buffers between passes: none, one pair, or two that alternate
    return to_align(segments * ntiles * TO_RADIX * (int64_t)sizeof(uint32_t)) + (pairs > 2 ? 2 : pairs) * 2 * to_align(n * 4);
}

extern "C" int obte_token_order(const int64_t* ids, int64_t segments, int64_t seg_len, int64_t vocab, int32_t* order, void* ws,
                                obte_stream s) {
    OBTE_REQUIRE(ids && order && ws, "obte_token_order: null pointer");
    OBTE_REQUIRE(segments > 0 && seg_len > 0, "obte_token_order: bad shape (segments and seg_len must be positive)");
    OBTE_REQUIRE(vocab >= 1 && vocab <= (1ll << 17), "obte_token_order: vocab must be in 1 .. 2^17");
    OBTE_REQUIRE(to_shape_ok(segments, seg_len, vocab), "obte_token_order: segments * seg_len must be below 2^31");
    hipStream_t st = (hipStream_t)s;
    const int64_t n = segments * seg_len, ntiles = cdiv64(seg_len, TO_TILE), nblocks = segments * ntiles;
    const int passes = to_passes(vocab);
    char* p = (char*)ws;
    uint32_t* hist = (uint32_t*)p;
    p += to_align(nblocks * TO_RADIX * (int64_t)sizeof(uint32_t));
    uint32_t* kbuf[2];
    int32_t* ibuf[2];
    for (int i = 0; i < 2; ++i) {   // the second pair is only touched (and only part of ws) when there are three passes
        kbuf[i] = (uint32_t*)p; p += to_align(n * 4);
        ibuf[i] = (int32_t*)p; p += to_align(n * 4);
    }
    ToShape sh;
    sh.seg_len = seg_len; sh.ntiles = ntiles;
    sh.keymask = passes * 8 >= 32 ? 0xffffffffu : ((1u << (passes * 8)) - 1u);
    for (int pass = 0; pass < passes; ++pass) {
        sh.shift = 8 * pass;
        const bool first = pass == 0, last = pass == passes - 1;
        const int64_t* src_ids = first ? ids : nullptr;
        const uint32_t* kin = first ? nullptr : kbuf[(pass - 1) & 1];
        const int32_t* iin = first ? nullptr : ibuf[(pass - 1) & 1];
        hipLaunchKernelGGL(token_hist_kernel, dim3((unsigned)nblocks), dim3(TO_THREADS), 0, st, src_ids, kin, hist, sh);
        OBTE_CHECK_LAUNCH("obte_token_order(hist)");
        hipLaunchKernelGGL(token_scan_kernel, dim3((unsigned)segments), dim3(TO_RADIX), 0, st, hist, ntiles);
        OBTE_CHECK_LAUNCH("obte_token_order(scan)");
        hipLaunchKernelGGL(token_scatter_kernel, dim3((unsigned)nblocks), dim3(TO_THREADS), 0, st, src_ids, kin, iin,
                           (const uint32_t*)hist, last ? (uint32_t*)nullptr : kbuf[pass & 1], last ? order : ibuf[pass & 1], sh);
        OBTE_CHECK_LAUNCH("obte_token_order(scatter)");
    }
    return OBTE_OK;
}

// =============================================================================================== causal bounds
// Elementwise: thread i owns position (b, t) as a QUERY (its key range, cut at t + 1) and as a KEY (the queries that see it: from
// t on, to the end of its document).  One 8-byte store per table and position.  An empty result is written as [x, x).
__global__ __launch_bounds__(256) void causal_bounds_kernel(const int32_t* __restrict__ doc, int64_t n, int T, int32_t* __restrict__ kr,
                                                            int32_t* __restrict__ qb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int t = (int)(i % T);
    int lo = 0, hi = T;
    if (doc) {
        const int2 d = *reinterpret_cast<const int2*>(doc + 2 * i);
        lo = max(d.x, 0); hi = min(d.y, T);
    }
    const int k_lo = lo, k_hi = min(hi, t + 1);   // as a query: the keys of its document up to itself
    const int q_lo = max(lo, t), q_hi = hi;       // as a key: the queries of its document from itself on
    *reinterpret_cast<int2*>(kr + 2 * i) = make_int2(k_lo, k_hi > k_lo ? k_hi : k_lo);
    *reinterpret_cast<int2*>(qb + 2 * i) = make_int2(q_lo, q_hi > q_lo ? q_hi : q_lo);
}

extern "C" int obte_causal_bounds(const int32_t* doc_ranges, int64_t B, int64_t T, int32_t* key_ranges, int32_t* query_bounds, obte_stream s) {
    OBTE_REQUIRE(key_ranges && query_bounds, "obte_causal_bounds: null pointer");
    OBTE_REQUIRE_ALIGNED("obte_causal_bounds", doc_ranges, "doc_ranges", 8);
    OBTE_REQUIRE_ALIGNED("obte_causal_bounds", key_ranges, "key_ranges", 8);
    OBTE_REQUIRE_ALIGNED("obte_causal_bounds", query_bounds, "query_bounds", 8);
    OBTE_REQUIRE(B > 0 && B < (1ll << 31) && T > 0 && T < (1ll << 24), "obte_causal_bounds: bad shape (1 <= B < 2^31, 1 <= T < 2^24)");
    OBTE_REQUIRE(doc_ranges != key_ranges && doc_ranges != query_bounds && key_ranges != query_bounds, "obte_causal_bounds: the tables must not alias");
    const int64_t n = B * T;
    OBTE_REQUIRE((n + 255) / 256 < (1ll << 31), "obte_causal_bounds: B * T too large for one launch");
    hipLaunchKernelGGL(causal_bounds_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, doc_ranges, n, (int)T, key_ranges, query_bounds);
    OBTE_CHECK_LAUNCH("obte_causal_bounds");
    return OBTE_OK;
}
