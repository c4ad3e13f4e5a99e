// bf16 GEMM on CDNA4 MFMA (v_mfma_f32_16x16x32_bf16), fp32 accumulate, bf16 output with fused epilogues.
// Second structure (default): 256x128 output tile per 512-thread workgroup, three LDS stages, loads two K-tiles
// ahead.
//
// Replaces the nn.Linear calls of the reference's block and readout (training/model.py:102,151,163,166,253)
// in all three passes: forward (A,B k-contiguous), dgrad (B k-strided), wgrad (A and B k-strided).
//
// Why this shape: the first structure (128x128, two stages, vmcnt(0) + barrier per K-step) measured ~3000 cycles
// per K-step against 512 cycles of MFMA work per wave — every step waited for its own LDS-DMA round trip.  Here
//   * 8 waves (4 along M x 2 along N, 64x64 each) share one 256x128 tile: two waves per SIMD, one workgroup per CU;
//   * the LDS ring holds three K-tiles (3 x 48 KiB); tile t+2 is issued right after the barrier that opens
//     step t, so each LDS-DMA piece has two full steps (>= 2 x 1024 MFMA cycles per SIMD) to land;
//   * the only wait in the loop is a COUNTED s_waitcnt vmcnt(6) (= the six pieces of tile t+1 stay in flight)
//     followed by a raw s_barrier — never vmcnt(0), never __syncthreads() (whose fence would drain the DMA);
//   * all LDS lives in one extern array (a second __shared__ object makes hipcc drain vmcnt before ds_reads).
// LDS images and swizzles (bank-conflict-free fragment reads; LDS-DMA writes linearly, so the permutation is
// applied to each lane's SOURCE address and again on the read):
//   k-contiguous operand : [rows][64 k], 128-B rows, 16-B chunk c of row r at c ^ ((r>>1)&7); ds_read_b128.
//   k-strided operand    : [64 k][mn], 512-B (A) / 256-B (B) rows, chunk c of k-row r at c ^ f(r),
//                          f(r) = ((r&3) | ((r>>3)&1)<<2) << 1; ds_read_b64_tr_b16 (hardware transpose).
// The MFMA is issued with swapped operands (C^T tiles) so each lane holds four consecutive output columns; the
// tile is staged through LDS and written in 16-B pieces of full 128-B row segments, applying the epilogue.
// Split-K (for weight gradients whose output has fewer tiles than the chip has CUs): each split writes an fp32
// partial tile to a slab; a second kernel sums the splits in a fixed order (bitwise reproducible) and rounds once.
#include "gemm_common.h"

namespace obte_gemm_v2 {

// OBTE_EPI_ACC32's arithmetic, each operation rounded on its own (a fused multiply-add would round alpha * acc + old once and the
// buffer's bits would depend on what the compiler fused): c = fl32(alpha * acc), sum = fl32(old + c)
__device__ __forceinline__ f32x4 acc32_term(f32x4 acc, float alpha) {
#pragma clang fp contract(off)
    return acc * alpha;
}
__device__ __forceinline__ f32x4 acc32_sum(f32x4 old, f32x4 c) {
#pragma clang fp contract(off)
    return old + c;
}

// Tile epilogue shared by both main-loop structures: stage the accumulators through LDS, apply EPI, write 16-B pieces.
template <int EPI, bool SPLIT, int BN>
__device__ __forceinline__ void tile_epilogue(const GemmParams& p, f32x4 (&acc)[BN / 32][4], char* smem, int wave, int lane,
                                              int64_t m0, int64_t n0, int wm, int wn, int split, int tile_n = BN) {
    constexpr int NJ = BN / 32, NW = BN / 2;
    __syncthreads();  // all fragment reads done (and no DMA outstanding): LDS becomes the epilogue staging area
    OBTE_GSTAMP(p, 5);

    const int em = lane & 15, en = (lane >> 4) * 4;
    if (SPLIT) {
        // fp32 partial tile -> slab[split][M][N]
        // 64 columns at a time through a per-wave fp32 staging area (8 x 17 KiB fits both tile widths)
        char* stg = smem + wave * (64 * EPI_LD_F32);
        float* out = p.slab + (int64_t)split * p.M * p.N;
#pragma unroll
        for (int half = 0; half < NJ / 4; ++half) {
            if (half) __syncthreads();
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    *reinterpret_cast<f32x4*>(stg + (mi * 16 + em) * EPI_LD_F32 + (ni * 16 + en) * 4) = acc[half * 4 + ni][mi];
            __syncthreads();
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                const int row = it * 4 + (lane >> 4);
                const int c4 = lane & 15;
                const int64_t m = m0 + wm * 64 + row;
                const int64_t n = n0 + wn * NW + half * 64 + c4 * 4;
                if (m < p.store_rows && n < p.N)
                    *reinterpret_cast<f32x4*>(out + m * p.N + n) = *reinterpret_cast<const f32x4*>(stg + row * EPI_LD_F32 + c4 * 16);
            }
        }
        return;
    }

    if (EPI == OBTE_EPI_ACC32) {
        // The weight gradient summed in fp32 over the passes of a step: the split-K staging above (64 columns at a time, 16-byte fp32
        // row chunks), with a read-modify-write of the caller's [M, N] fp32 buffer in place of the slab store and, on the last pass,
        // the bf16 gradient written from the sum already in registers.  acc32_mode is uniform (one problem, one mode).  ldd == N
        // (host-checked): one offset serves acc32 and d.  Interior tiles issue the eight loads of a batch before its first store
        // (vmcnt retires in order: a load behind a store waits for the store) and address with one 64-bit tile origin plus 32-bit
        // in-tile offsets, as the bf16 path below; two batches per half keep the loaded chunks to 32 registers beside the accumulators.
        char* stg = smem + wave * (64 * EPI_LD_F32);
        const int mode = p.acc32_mode;
        const bool interior = m0 + BM <= p.store_rows && n0 + tile_n <= p.N;
        const int64_t tile_o = m0 * p.N + n0;
        const uint32_t n32 = (uint32_t)p.N;
        const uint32_t off_l = (uint32_t)(wm * 64 + (lane >> 4)) * n32 + (uint32_t)(wn * NW + (lane & 15) * 4);
#pragma unroll
        for (int half = 0; half < NJ / 4; ++half) {
            if (half) __syncthreads();
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    *reinterpret_cast<f32x4*>(stg + (mi * 16 + em) * EPI_LD_F32 + (ni * 16 + en) * 4) = acc[half * 4 + ni][mi];
            __syncthreads();
            if (interior) {
#pragma unroll
                for (int b8 = 0; b8 < 2; ++b8) {
                    f32x4 old[8];
                    if (mode != OBTE_ACC32_FIRST) {
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            old[i] = *reinterpret_cast<const f32x4*>(p.acc32 + tile_o + (int64_t)(off_l + (uint32_t)(half * 64) + (uint32_t)((b8 * 8 + i) * 4) * n32));
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int it = b8 * 8 + i;
                        const int64_t o = tile_o + (int64_t)(off_l + (uint32_t)(half * 64) + (uint32_t)(it * 4) * n32);
                        f32x4 v = acc32_term(*reinterpret_cast<const f32x4*>(stg + (it * 4 + (lane >> 4)) * EPI_LD_F32 + (lane & 15) * 16), p.alpha);
                        if (mode != OBTE_ACC32_FIRST) v = acc32_sum(old[i], v);
                        *reinterpret_cast<f32x4*>(p.acc32 + o) = v;
                        if (mode == OBTE_ACC32_LAST) *reinterpret_cast<bf16x4*>(p.d + o) = __builtin_convertvector(v, bf16x4);
                    }
                }
            } else {
#pragma unroll
                for (int it = 0; it < 16; ++it) {
                    const int row = it * 4 + (lane >> 4);
                    const int c4 = lane & 15;
                    const int64_t m = m0 + wm * 64 + row;
                    const int64_t n = n0 + wn * NW + half * 64 + c4 * 4;
                    if (m < p.store_rows && n < p.N) {
                        const int64_t o = m * p.N + n;
                        f32x4 v = acc32_term(*reinterpret_cast<const f32x4*>(stg + row * EPI_LD_F32 + c4 * 16), p.alpha);
                        if (mode != OBTE_ACC32_FIRST) v = acc32_sum(*reinterpret_cast<const f32x4*>(p.acc32 + o), v);
                        *reinterpret_cast<f32x4*>(p.acc32 + o) = v;
                        if (mode == OBTE_ACC32_LAST) *reinterpret_cast<bf16x4*>(p.d + o) = __builtin_convertvector(v, bf16x4);
                    }
                }
            }
        }
        return;
    }

    // staged row: NW bf16 + 16 B pad (144 B for the 64-wide wave tile, 208 B for the 96-wide, 272 B for the 128-wide one)
    constexpr int LDE = NW * 2 + 16;
    constexpr int CPRE = NW / 8;            // 16-B chunks per staged row
    // the wave's 64 x NW tile leaves as 64 * CPRE 16-byte chunks, 64 per wave-wide access: chunk 64 it + lane = (row, c8).  For a
    // power-of-two CPRE that is rows it * (64 / CPRE) + lane / CPRE of one column chunk per lane; the 96-wide wave tile
    // (BN = 192, CPRE = 12) walks rows and columns together.
    constexpr int NIT = CPRE;
    auto chunk_row = [&](int it) { return (64 * it + lane) / CPRE; };
    auto chunk_c8 = [&](int it) { return (64 * it + lane) % CPRE; };
    char* stg = smem + wave * (64 * LDE);
#pragma unroll
    for (int ni = 0; ni < NJ; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)   // (as one vector conversion: two v_pk_mul + two v_cvt_pk per quad; element by element hipcc emitted ten instructions)
            *reinterpret_cast<bf16x4*>(stg + (mi * 16 + em) * LDE + (ni * 16 + en) * 2) =
                __builtin_convertvector((EPI == OBTE_EPI_NONE || EPI == OBTE_EPI_ADD) ? acc[ni][mi] * p.alpha : acc[ni][mi], bf16x4);   // (alpha != 1 only with these two: validate_args)
    // Interior tiles whose epilogue READS global memory (residual / gradient accumulation, GELU', dropout + residual, RoPE
    // tables) take a branch-free path that issues every one of those loads BEFORE the first store.  In the guarded loop below
    // each iteration is load -> s_waitcnt vmcnt(0) -> arithmetic -> store behind a bounds branch hipcc does not schedule
    // across, and vmcnt retires in issue order: every load waited for the previous iteration's STORE to reach memory — 16
    // dependent round trips per tile (c_fc dgrad + GELU': 38 of its 103 us were this epilogue).
    constexpr bool READS = EPI == OBTE_EPI_ADD || EPI == OBTE_EPI_GELU_BWD || EPI == OBTE_EPI_ADD_DROPOUT || EPI == OBTE_EPI_ROPE_QK;
    const bool interior = m0 + BM <= p.store_rows && n0 + tile_n <= p.N && (EPI != OBTE_EPI_ADD || p.aux != nullptr);
    if (interior) {   // (the epilogues without loads take it too: no bounds branches, so the staged reads are issued ahead of the arithmetic)
        // output offset and column of chunk `it`: for a power-of-two CPRE the lane keeps its column and steps 64 / CPRE rows
        // Addresses: ONE 64-bit tile origin per workgroup (scalar) and 32-bit element offsets inside the tile (< 256 rows x ldd) — the
        // 64-bit per-chunk products this replaced were v_mad_u64_u32 / v_mul_lo_u32 at quarter rate, 66 of them per wave and tile
        // (a CU stores a 128-KB tile in ~0.8 us when it does nothing else, tools/micro/store_path.hip; this epilogue takes 4.1 us,
        // most of it latency chains between its phases — trimming its instructions did not change that: DESIGN 10.2)
        constexpr bool POW2 = (CPRE & (CPRE - 1)) == 0;
        const int64_t tile_o = m0 * p.ldd + n0;
        const uint32_t ldd32 = (uint32_t)p.ldd;
        const uint32_t nc_l = (uint32_t)(wn * NW + (lane % CPRE) * 8);                 // column inside the tile
        const uint32_t off_l = (uint32_t)(wm * 64 + lane / CPRE) * ldd32 + nc_l;
        auto nn_of = [&](int it) { return n0 + (POW2 ? nc_l : (uint32_t)(wn * NW + chunk_c8(it) * 8)); };
        auto oo_of = [&](int it) {
            const uint32_t off = POW2 ? off_l + (uint32_t)(it * (64 / CPRE)) * ldd32
                                      : (uint32_t)(wm * 64 + chunk_row(it)) * ldd32 + (uint32_t)(wn * NW + chunk_c8(it) * 8);
            return tile_o + (int64_t)off;
        };
        bf16x8 r[NIT];
        f32x4 rc[NIT], rs[NIT];
        if (EPI == OBTE_EPI_ROPE_QK) {
            const uint32_t T32 = (uint32_t)p.rope_T, hs32 = (uint32_t)p.rope_hs;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {   // lanes on the v third load the same (valid) table rows and leave their values alone
                const uint32_t nu = (uint32_t)nn_of(it);
                const uint32_t dd = (hs32 & (hs32 - 1)) == 0 ? (nu & (hs32 - 1)) : (nu % hs32);
                const uint32_t mu = (uint32_t)(m0 + wm * 64 + chunk_row(it));
                const uint32_t t = (T32 & (T32 - 1)) == 0 ? (mu & (T32 - 1)) : (mu % T32);
                rc[it] = *reinterpret_cast<const f32x4*>(p.rope_cos + t * (hs32 / 2) + dd / 2);
                rs[it] = *reinterpret_cast<const f32x4*>(p.rope_sin + t * (hs32 / 2) + dd / 2);
            }
        } else if (READS) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) r[it] = *reinterpret_cast<const bf16x8*>(p.aux + oo_of(it));
        }
        // (no barrier here: a wave reads back exactly the 64 x NW region it staged itself, and one wave's LDS operations execute
        //  in order — the barrier at the top, which keeps the staging off ring stages other waves may still be reading, is the only
        //  one the epilogue needs)
        OBTE_GSTAMP(p, 6);
        // every staged chunk into registers first (the accumulators' registers are free now): the non-temporal store below is an asm
        // statement with a memory clobber, and with the LDS read inside its loop hipcc kept each read behind the previous store —
        // sixteen LDS round trips in a row per wave
        bf16x8 staged[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) staged[it] = *reinterpret_cast<const bf16x8*>(stg + chunk_row(it) * LDE + chunk_c8(it) * 16);
#ifdef OBTE_DEBUG_HOOKS
        if (p.dbg_times) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); OBTE_GSTAMP(p, 7); }
#endif
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            bf16x8 v = staged[it];
            const int64_t o = oo_of(it);
            const int64_t n = nn_of(it);
            const bool rot = n < 2 * (p.N / 3);
            if (EPI == OBTE_EPI_GELU) {
                bf16x8 g;
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    f32x2_t act, der;
                    gelu_ref_both2(f32x2_t{bf2f(v[j]), bf2f(v[j + 1])}, act, der);
                    g[j] = f2bf(act[0]); g[j + 1] = f2bf(act[1]);
                    v[j] = f2bf(der[0]); v[j + 1] = f2bf(der[1]);
                }
                *reinterpret_cast<bf16x8*>(p.d2 + o) = g;
            } else if (EPI == OBTE_EPI_GELU_ACT) {
                v = gelu_act8(v);   // the activation alone (a forward without a backward): one output, stored as any other d
            } else if (EPI == OBTE_EPI_ADD) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = f2bf(bf2f(r[it][j]) + bf2f(v[j]));
            } else if (EPI == OBTE_EPI_GELU_BWD) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = f2bf(bf2f(v[j]) * bf2f(r[it][j]));
            } else if (EPI == OBTE_EPI_ROPE_QK) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float xe = bf2f(v[2 * j]), xo = bf2f(v[2 * j + 1]);
                    const bf16 ne = f2bf(xe * rc[it][j] - xo * rs[it][j]), no = f2bf(xe * rs[it][j] + xo * rc[it][j]);
                    v[2 * j] = rot ? ne : v[2 * j];
                    v[2 * j + 1] = rot ? no : v[2 * j + 1];
                }
            } else if (EPI == OBTE_EPI_ADD_DROPOUT) {
                const int64_t m = m0 + wm * 64 + chunk_row(it);
                const uint32_t rk = drop_rowkey((uint64_t)m, p.drop);   // dropout element = (row m, column n + j)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const uint32_t bits = drop_pair_bits(rk, (uint32_t)(n >> 1) + jj);
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int j = 2 * jj + e;
                        const float t = drop_keep_bits(bits, (uint32_t)e, p.drop) ? bf2f(f2bf(bf2f(v[j]) * p.drop.scale)) : 0.f;
                        v[j] = f2bf(bf2f(r[it][j]) + t);
                    }
                }
            }
            if (p.nt_store) asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" : : "v"(p.d + o), "v"(v) : "memory");   // (s_nop: an asm store of more than 8 bytes must not be followed at once by a write of its data registers; hipcc pads only its own stores)
            else *reinterpret_cast<bf16x8*>(p.d + o) = v;
        }
        return;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int row = chunk_row(it);
        const int c8 = chunk_c8(it);
        const int64_t m = m0 + wm * 64 + row;
        const int64_t n = n0 + wn * NW + c8 * 8;
        if (m < p.store_rows && n < p.N) {
            bf16x8 v = *reinterpret_cast<const bf16x8*>(stg + row * LDE + c8 * 16);
            const int64_t o = m * p.ldd + n;
            if (EPI == OBTE_EPI_GELU) {
                // one erf/exp evaluation yields both the activation (d2) and its derivative (d): the backward
                // epilogue is then a plain multiply
                bf16x8 g;
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    f32x2_t act, der;
                    gelu_ref_both2(f32x2_t{bf2f(v[j]), bf2f(v[j + 1])}, act, der);
                    g[j] = f2bf(act[0]); g[j + 1] = f2bf(act[1]);
                    v[j] = f2bf(der[0]); v[j + 1] = f2bf(der[1]);
                }
                *reinterpret_cast<bf16x8*>(p.d2 + o) = g;
            } else if (EPI == OBTE_EPI_GELU_ACT) {
                v = gelu_act8(v);
            } else if (EPI == OBTE_EPI_ADD) {
                if (p.aux) {   // uniform; null only inside a mixed group (a problem without accumulation)
                    const bf16x8 r = *reinterpret_cast<const bf16x8*>(p.aux + o);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = f2bf(bf2f(r[j]) + bf2f(v[j]));
                }
            } else if (EPI == OBTE_EPI_ROPE_QK) {
                // packed c_attn output [.., 3C]: rotate the (even, odd) pairs of the q and k thirds (columns < 2N/3),
                // position = row % T; the v third passes through.  fp32 arithmetic on the bf16-rounded projection.
                if (n < 2 * (p.N / 3)) {
                    // position and in-head column by 32-bit arithmetic, masks when T / head_dim are powers of two (uniform
                    // branches): the 64-bit `%` this replaced was a software division per 16-byte chunk — 9 to 22 us of
                    // the 65-us c_attn GEMM
                    const uint32_t mu = (uint32_t)m, nu = (uint32_t)n, T32 = (uint32_t)p.rope_T, hs32 = (uint32_t)p.rope_hs;
                    const uint32_t t = (T32 & (T32 - 1)) == 0 ? (mu & (T32 - 1)) : (mu % T32);
                    const uint32_t dd = (hs32 & (hs32 - 1)) == 0 ? (nu & (hs32 - 1)) : (nu % hs32);
                    const f32x4 c = *reinterpret_cast<const f32x4*>(p.rope_cos + t * (hs32 / 2) + dd / 2);
                    const f32x4 sn = *reinterpret_cast<const f32x4*>(p.rope_sin + t * (hs32 / 2) + dd / 2);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float xe = bf2f(v[2 * j]), xo = bf2f(v[2 * j + 1]);
                        v[2 * j] = f2bf(xe * c[j] - xo * sn[j]);
                        v[2 * j + 1] = f2bf(xe * sn[j] + xo * c[j]);
                    }
                }
            } else if (EPI == OBTE_EPI_ADD_DROPOUT) {
                const bf16x8 r = *reinterpret_cast<const bf16x8*>(p.aux + o);
                const uint32_t rk = drop_rowkey((uint64_t)m, p.drop);   // dropout element = (row m, column n + j)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const uint32_t bits = drop_pair_bits(rk, (uint32_t)(n >> 1) + jj);
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int j = 2 * jj + e;
                        const float t = drop_keep_bits(bits, (uint32_t)e, p.drop) ? bf2f(f2bf(bf2f(v[j]) * p.drop.scale)) : 0.f;
                        v[j] = f2bf(bf2f(r[j]) + t);
                    }
                }
            } else if (EPI == OBTE_EPI_GELU_BWD) {
                const bf16x8 h = *reinterpret_cast<const bf16x8*>(p.aux + o);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = f2bf(bf2f(v[j]) * bf2f(h[j]));
            }
            // an output larger than the Infinity Cache (the 1-GiB logits) is stored non-temporally: it cannot stay on
            // die for its consumer anyway, and this way it does not evict the operand panels the XCD's other
            // workgroups are still streaming from L2 (+7 % on the readout forward; smaller outputs measured slower)
            if (p.nt_store) asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" : : "v"(p.d + o), "v"(v) : "memory");   // (s_nop: an asm store of more than 8 bytes must not be followed at once by a write of its data registers; hipcc pads only its own stores)   // (the builtin form is folded into the plain store below)
            else *reinterpret_cast<bf16x8*>(p.d + o) = v;
        }
    }
}

template <bool A_KMAJOR, bool B_KMAJOR, int EPI, bool SPLIT, int BN>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_v2_kernel(GemmParams p) {
    using CF = Cfg<BN>;
    constexpr int NJ = CF::NJ, NPB = CF::NPB, STAGE_BYTES = CF::STAGE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (p.store_rows < 0) return;   // timing-only diagnostic: launch cost of the empty grid
    OBTE_GSTAMP(p, 0);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;

    // ---- workgroup -> (tile, split): bijective XCD remap, then 8-row groups of tiles ------------------------
    const int nwg = p.tiles_m * p.tiles_n * p.splits;
    const int bid = blockIdx.x;
    const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    const int split = wgid % p.splits;
    const int tid_ = wgid / p.splits;
    const int group_sz = 8 * p.tiles_n;
    const int first_m = (tid_ / group_sz) * 8;
    const int gsz = min(p.tiles_m - first_m, 8);
    const int tm = first_m + (tid_ % group_sz) % gsz;
    const int tn = (tid_ % group_sz) / gsz;
    const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
    int voff_a[4], voff_b[NPB];
    dma_offsets<A_KMAJOR, BM, 4>(wave, lane, p.lda, voff_a);
    dma_offsets<B_KMAJOR, BN, NPB>(wave, lane, p.ldb, voff_b);

    const int wm = wave >> 1, wn = wave & 1;
    f32x4 acc[NJ][4];
#pragma unroll
    for (int i = 0; i < NJ; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk_total = (int)((p.K + BKT - 1) / BKT);
    const int kt0 = split * p.k_per_split;
    const int nk = min(p.k_per_split, nk_total - kt0);

    auto issue = [&](int t, int stage) {
        const int64_t k0 = (int64_t)(kt0 + t) * BKT;
        const int64_t ao = A_KMAJOR ? (m0 * p.lda + k0) : (k0 * p.lda + m0);
        const int64_t bo = B_KMAJOR ? (n0 * p.ldb + k0) : (k0 * p.ldb + n0);
        char* st = smem + stage * STAGE_BYTES;
        dma_tile<4>(p.a + ao, p.a_elems - ao, voff_a, st, wave);
        dma_tile<NPB>(p.b + bo, p.b_elems - bo, voff_b, st + A_TILE, wave);
    };

    // ---- main loop, software pipelined over half K-tiles -------------------------------------------------------
    // Each K-tile (64) is two MFMA k-steps; fragments are double-buffered in registers (F0: k-step 0, F1: k-step 1).
    //   step t:  [3-stage ring: issue DMA of tile t+2]  read F1(t) | MFMA F0(t) | wait tile t+1, barrier |
    //            read F0(t+1)  [2-stage ring: issue DMA of tile t+2]  | MFMA F1(t)
    // so every LDS fragment read and every DMA issue runs under 32 (or 16) MFMAs of the same wave, there is one
    // barrier per K-tile, and the DMA waits are counted (3-stage: the six pieces of tile t+2 stay in flight).
    // sched_barrier pins this order; left alone hipcc sinks each ds_read to just before its first use.
    auto stage_of = [&](int t) { return CF::NSTAGE == 3 ? t % 3 : (t & 1); };
    auto load_frags = [&](int t, int ks, bf16x8 (&af)[4], bf16x8 (&bfr)[NJ]) {
        const char* ta = smem + stage_of(t) * STAGE_BYTES;
        const char* tb = ta + A_TILE;
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = load_frag<A_KMAJOR, BM>(ta, wm * 64 + i * 16, ks, lane);
#pragma unroll
        for (int i = 0; i < NJ; ++i) bfr[i] = load_frag<B_KMAJOR, BN>(tb, wn * (BN / 2) + i * 16, ks, lane);
    };
    auto mma = [&](const bf16x8 (&af)[4], const bf16x8 (&bfr)[NJ]) {
#pragma unroll
        for (int ni = 0; ni < NJ; ++ni)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                // operands swapped: the accumulator holds C^T (row = n, col = m)
                acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[ni][mi], 0, 0, 0);
    };

    bf16x8 a0[4], b0[NJ], a1[4], b1[NJ];
    if (nk > 0) {
        issue(0, 0);
        if (nk > 1) issue(1, 1);
        if (CF::NSTAGE == 3 && nk > 1) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else if (CF::NSTAGE == 2 && nk > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 + NPB) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        OBTE_GSTAMP(p, 1);
        load_frags(0, 0, a0, b0);
    }
    for (int t = 0; t + 1 < nk; ++t) {
        if (CF::NSTAGE == 3 && t + 2 < nk) issue(t + 2, (t + 2) % 3);   // stage of tile t-1: free since the last barrier
        load_frags(t, 1, a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        mma(a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        // the builtin form (not inline asm) so that hipcc's own wait bookkeeping knows F1 has landed and does not
        // make MFMA F1 wait behind the F0(t+1) reads issued below.  simm16: vmcnt[3:0], expcnt 7, lgkmcnt 0.
        if (CF::NSTAGE == 3 && t + 2 < nk) __builtin_amdgcn_s_waitcnt(0x0076);   // vmcnt(6) lgkmcnt(0)
        else __builtin_amdgcn_s_waitcnt(0x0070);                                  // vmcnt(0) lgkmcnt(0)
        __builtin_amdgcn_s_barrier();   // tile t+1 landed for everyone; everyone holds tile t's fragments in registers
        load_frags(t + 1, 0, a0, b0);
        if (CF::NSTAGE == 2 && t + 2 < nk) issue(t + 2, t & 1);
        __builtin_amdgcn_sched_barrier(0);
        mma(a1, b1);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (nk > 0) {   // last K-tile: nothing left to fetch
        load_frags(nk - 1, 1, a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        mma(a0, b0);
        mma(a1, b1);
    }
    OBTE_GSTAMP(p, 2);
    tile_epilogue<EPI, SPLIT, BN>(p, acc, smem, wave, lane, m0, n0, wm, wn, split);
#ifdef OBTE_DEBUG_HOOKS
    OBTE_GSTAMP(p, 3);
    if (p.dbg_times) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); OBTE_GSTAMP(p, 4); }
#endif
}

// Explicit instantiations: with implicit instantiation alone hipcc (ROCm 7.2) emitted the host stub of only the
// first specialisation it met; the library then failed to load with undefined kernel symbols.
#define OBTE_INST(AK, BK, BN)                                                                    \
    template __global__ void gemm_v2_kernel<AK, BK, OBTE_EPI_NONE, true, BN>(GemmParams);        \
    template __global__ void gemm_v2_kernel<AK, BK, OBTE_EPI_NONE, false, BN>(GemmParams);       \
    template __global__ void gemm_v2_kernel<AK, BK, OBTE_EPI_GELU, false, BN>(GemmParams);       \
    template __global__ void gemm_v2_kernel<AK, BK, OBTE_EPI_ADD, false, BN>(GemmParams);        \
    template __global__ void gemm_v2_kernel<AK, BK, OBTE_EPI_GELU_BWD, false, BN>(GemmParams);      \
    template __global__ void gemm_v2_kernel<AK, BK, OBTE_EPI_ADD_DROPOUT, false, BN>(GemmParams);   \
    template __global__ void gemm_v2_kernel<AK, BK, OBTE_EPI_ROPE_QK, false, BN>(GemmParams);
OBTE_INST(true, true, 128)
template __global__ void gemm_v2_kernel<true, true, OBTE_EPI_GELU_ACT, false, 128>(GemmParams);   // (x W^T only)
template __global__ void gemm_v2_kernel<true, true, OBTE_EPI_GELU_ACT, false, 256>(GemmParams);
OBTE_INST(true, false, 128)
OBTE_INST(false, true, 128)
OBTE_INST(false, false, 128)
OBTE_INST(true, true, 256)
OBTE_INST(true, false, 256)
OBTE_INST(false, true, 256)
OBTE_INST(false, false, 256)
#undef OBTE_INST
template __global__ void gemm_v2_kernel<false, false, OBTE_EPI_ACC32, false, 128>(GemmParams);   // (the weight-gradient layout only)
template __global__ void gemm_v2_kernel<false, false, OBTE_EPI_ACC32, false, 256>(GemmParams);
// BN = 192: k-contiguous operands only (the forward projections), no split-K.  For outputs whose width is a multiple of 192 but
// leaves the 256-wide tiling a ragged last round — c_attn at the small config: N = 3072 is 384 tiles of 256 x 256 = 1.5 rounds of
// the 256 CUs, and 512 tiles of 256 x 192 = two full ones (a quarter less work per round).
#define OBTE_INST192(EPI) template __global__ void gemm_v2_kernel<true, true, EPI, false, 192>(GemmParams);
OBTE_INST192(OBTE_EPI_NONE) OBTE_INST192(OBTE_EPI_GELU) OBTE_INST192(OBTE_EPI_ADD) OBTE_INST192(OBTE_EPI_ADD_DROPOUT) OBTE_INST192(OBTE_EPI_ROPE_QK) OBTE_INST192(OBTE_EPI_GELU_ACT)
#undef OBTE_INST192

// ---- third structure: 256x256 tile, ring of FOUR half K-tiles (32 k each, 32 KiB), loads three half-steps ahead ----
// The 2-stage ring above keeps at most one 64-KiB K-tile in flight per CU and each burst has to complete inside one
// iteration; measured, an iteration then lasts as long as one burst's round trip (~2 us: every line of a tile is a
// first touch for its L2, so each burst sees the beyond-L2 latency).  Splitting the ring into 32-k half-stages lets the
// refill of a slot start as soon as ITS fragments are in registers: three half-stages (96 KiB) are in flight in
// steady state and each has three half-steps (1.5 K-tiles of MFMA work) to land.  One barrier per half-step.
//   step u:  wait half-stage u+1 (vmcnt(8): u+2, u+3 stay in flight) | barrier | 4 x { read 3 fragments of F(u+1),
//            issue one LDS-DMA piece of u+4 -> slot u&3, 8 MFMAs of F(u) }
// The LDS-DMA is issued through inline asm (common.h lds_dma16): with the builtin, hipcc put an s_waitcnt vmcnt(0) in
// front of every transposing LDS read, i.e. drained the whole ring at each half-step for the k-strided layouts.
// k-contiguous half image: [256 rows][32 k], 64-B rows, chunk c of row r at c ^ ((4 - (r>>2)) & 3) (conflict-free
// ds_read_b128 for the 16x32 fragment); k-strided half image: [32 k][256], as above.
// one 256x256 tile (or K-split of it) of problem p; wgid in [0, tiles_m * tiles_n * splits)
template <bool A_KMAJOR, bool B_KMAJOR, int EPI, bool SPLIT>
__device__ __forceinline__ void v3_tile(const GemmParams& p, const int wgid, char* smem) {
    constexpr int BN = 256, NJ = 8;
    OBTE_GSTAMP(p, 0);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int split = wgid % p.splits;
    const int tid_ = wgid / p.splits;
    const int group_sz = 8 * p.tiles_n;
    const int first_m = (tid_ / group_sz) * 8;
    const int gsz = min(p.tiles_m - first_m, 8);
    const int tm = first_m + (tid_ % group_sz) % gsz;
    const int tn = (tid_ % group_sz) / gsz;
    const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;

    int voff_a[2], voff_b[2];
    dma_offsets_h<A_KMAJOR>(wave, lane, p.lda, voff_a);
    dma_offsets_h<B_KMAJOR>(wave, lane, p.ldb, voff_b);

    const int wm = wave >> 1, wn = wave & 1;
    f32x4 acc[NJ][4];
#pragma unroll
    for (int i = 0; i < NJ; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk_total = (int)((p.K + BKT - 1) / BKT);
    const int kt0 = split * p.k_per_split;
    const int nh = 2 * min(p.k_per_split, nk_total - kt0);   // half-steps; even, >= 4 (checked by the host)

    auto issue = [&](int u) {
        const int64_t k0 = (int64_t)kt0 * BKT + (int64_t)u * 32;
        const int64_t ao = A_KMAJOR ? (m0 * p.lda + k0) : (k0 * p.lda + m0);
        const int64_t bo = B_KMAJOR ? (n0 * p.ldb + k0) : (k0 * p.ldb + n0);
        char* st = smem + (u & 3) * H_STAGE;
        dma_tile<2>(p.a + ao, p.a_elems - ao, voff_a, st, wave);
        dma_tile<2>(p.b + bo, p.b_elems - bo, voff_b, st + H_TILE, wave);
    };
    auto load_frags = [&](int u, bf16x8 (&af)[4], bf16x8 (&bfr)[NJ]) {
        const char* ta = smem + (u & 3) * H_STAGE;
        const char* tb = ta + H_TILE;
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = load_frag_h<A_KMAJOR>(ta, wm * 64 + i * 16, lane);
#pragma unroll
        for (int i = 0; i < NJ; ++i) bfr[i] = load_frag_h<B_KMAJOR>(tb, wn * 128 + i * 16, lane);
    };
    auto mma = [&](const bf16x8 (&af)[4], const bf16x8 (&bfr)[NJ]) {
#pragma unroll
        for (int ni = 0; ni < NJ; ++ni)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[ni][mi], 0, 0, 0);
    };

    bf16x8 a0[4], b0[NJ], a1[4], b1[NJ];
    issue(0); issue(1); issue(2); issue(3);
    __builtin_amdgcn_s_waitcnt(0x007C);   // vmcnt(12): half-stage 0 landed
    __builtin_amdgcn_s_barrier();
    OBTE_GSTAMP(p, 1);
    load_frags(0, a0, b0);
    int u = 0;
    // Steady state, hand-interleaved and pinned with sched_barrier: group g of half-step u = {A fragment g and
    // B fragments 2g, 2g+1 of half-step u+1, LDS-DMA piece g of half-step u+4 (slot u&3: every wave holds F(u) in
    // registers since the barrier), the 8 MFMAs of n sub-tiles 2g, 2g+1 of half-step u}.
    auto istep = [&](int uu, const bf16x8 (&af)[4], const bf16x8 (&bfr)[NJ], bf16x8 (&an)[4], bf16x8 (&bn)[NJ]) {
        const char* ta = smem + ((uu + 1) & 3) * H_STAGE;
        const char* tb = ta + H_TILE;
        const int64_t k0 = (int64_t)kt0 * BKT + (int64_t)(uu + 4) * 32;
        const int64_t ao = A_KMAJOR ? (m0 * p.lda + k0) : (k0 * p.lda + m0);
        const int64_t bo = B_KMAJOR ? (n0 * p.ldb + k0) : (k0 * p.ldb + n0);
        const i32x4_t ra = make_rsrc_words(p.a + ao, (p.a_elems - ao) * 2);
        const i32x4_t rb = make_rsrc_words(p.b + bo, (p.b_elems - bo) * 2);
        const uint32_t lds_st = lds_addr_of(smem + (uu & 3) * H_STAGE) + wave * 1024;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            an[g] = load_frag_h<A_KMAJOR>(ta, wm * 64 + g * 16, lane);
            bn[2 * g] = load_frag_h<B_KMAJOR>(tb, wn * 128 + (2 * g) * 16, lane);
            bn[2 * g + 1] = load_frag_h<B_KMAJOR>(tb, wn * 128 + (2 * g + 1) * 16, lane);
            if (g < 2) lds_dma16(ra, lds_st + 8 * g * 1024, voff_a[g]);
            else lds_dma16(rb, lds_st + H_TILE + 8 * (g - 2) * 1024, voff_b[g - 2]);
#pragma unroll
            for (int ni = 2 * g; ni < 2 * g + 2; ++ni)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[ni][mi], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    for (; u + 4 < nh; u += 2) {
        __builtin_amdgcn_s_waitcnt(0x0078);   // vmcnt(8) lgkmcnt(0): half-stage u+1 landed, F(u) reads complete
        __builtin_amdgcn_s_barrier();
        istep(u, a0, b0, a1, b1);
        __builtin_amdgcn_s_waitcnt(0x0078);
        __builtin_amdgcn_s_barrier();
        istep(u + 1, a1, b1, a0, b0);
    }
    // last four half-steps (u == nh - 4): nothing left to issue, the waits count down
    __builtin_amdgcn_s_waitcnt(0x0078);
    __builtin_amdgcn_s_barrier();
    load_frags(u + 1, a1, b1);
    __builtin_amdgcn_sched_barrier(0);
    mma(a0, b0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0x0074);       // vmcnt(4)
    __builtin_amdgcn_s_barrier();
    load_frags(u + 2, a0, b0);
    __builtin_amdgcn_sched_barrier(0);
    mma(a1, b1);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0x0070);       // vmcnt(0)
    __builtin_amdgcn_s_barrier();
    load_frags(u + 3, a1, b1);
    __builtin_amdgcn_sched_barrier(0);
    mma(a0, b0);
    mma(a1, b1);
    OBTE_GSTAMP(p, 2);
    tile_epilogue<EPI, SPLIT, BN>(p, acc, smem, wave, lane, m0, n0, wm, wn, split);
#ifdef OBTE_DEBUG_HOOKS
    OBTE_GSTAMP(p, 3);
    if (p.dbg_times) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); OBTE_GSTAMP(p, 4); }
#endif
}

template <bool A_KMAJOR, bool B_KMAJOR, int EPI, bool SPLIT>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_v3_kernel(GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    v3_tile<A_KMAJOR, B_KMAJOR, EPI, SPLIT>(p, xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n * p.splits), smem);
}

// Grouped launch: up to GROUP_MAX independent GEMMs in ONE grid of 256x256 tiles, each tile running its full K (no
// split-K).  Built for the backward pass of a transformer block: alone, none of its four weight gradients
// (dW = dY^T X, K = tokens) has enough tiles for 256 CUs, so each used to be a split-K launch plus a reduce kernel
// over fp32 slabs; together they have 192 tiles at n_embd = 1024 (768 at 2048), every tile accumulates straight into
// the gradient, and the slabs, the reduce launches and three kernel tails disappear.  The 64 CUs those 192 tiles leave
// idle are filled with the tiles of a SHORTER independent product of the same layer (the c_attn input gradient,
// 128 tiles of K = 3 n_embd): problems come in two classes — class 0 = the leading problems with the longest K,
// class 1 = the rest — and when both class sizes divide by 8 every XCD receives its share of class 0 first, then
// its share of class 1, so the short tiles start on the CUs that got no long one and behind the first finishers.
// Layout and accumulate/overwrite are per problem (uniform branches; aux == null means overwrite); a problem with OBTE_EPI_ACC32 (the
// weight-gradient layout) is dealt as a layout of its own.
// (GroupParams: gemm_common.h)
__global__ __launch_bounds__(NTHREADS, 2) void gemm_v3_group_kernel(GroupParams gp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nwg = gp.first_wg[GROUP_MAX];
    int wgid;
    if (gp.n_class0 > 0) {   // both class sizes are multiples of 8 (host-checked)
        const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
        const int c0 = gp.n_class0 >> 3, c1 = (nwg - gp.n_class0) >> 3;
        wgid = k < c0 ? xcd * c0 + k : gp.n_class0 + xcd * c1 + (k - c0);
    } else {
        wgid = xcd_remap(blockIdx.x, nwg);
    }
    int i = 0;
#pragma unroll
    for (int j = 1; j < GROUP_MAX; ++j) i += (wgid >= gp.first_wg[j]) ? 1 : 0;
    const int local = wgid - gp.first_wg[i];
    switch (gp.layout[i]) {
        case 0: v3_tile<false, false, OBTE_EPI_ADD, false>(gp.g[i], local, smem); break;
        case 1: v3_tile<false, true, OBTE_EPI_ADD, false>(gp.g[i], local, smem); break;
        case 2: v3_tile<true, false, OBTE_EPI_ADD, false>(gp.g[i], local, smem); break;
        case 3: v3_tile<true, true, OBTE_EPI_ADD, false>(gp.g[i], local, smem); break;
        default: v3_tile<false, false, OBTE_EPI_ACC32, false>(gp.g[i], local, smem); break;   // 4: a weight gradient summed in fp32 over passes
    }
}

#define OBTE_INST3(AK, BK)                                                                   \
    template __global__ void gemm_v3_kernel<AK, BK, OBTE_EPI_NONE, true>(GemmParams);        \
    template __global__ void gemm_v3_kernel<AK, BK, OBTE_EPI_NONE, false>(GemmParams);       \
    template __global__ void gemm_v3_kernel<AK, BK, OBTE_EPI_GELU, false>(GemmParams);       \
    template __global__ void gemm_v3_kernel<AK, BK, OBTE_EPI_ADD, false>(GemmParams);        \
    template __global__ void gemm_v3_kernel<AK, BK, OBTE_EPI_GELU_BWD, false>(GemmParams);   \
    template __global__ void gemm_v3_kernel<AK, BK, OBTE_EPI_ADD_DROPOUT, false>(GemmParams); \
    template __global__ void gemm_v3_kernel<AK, BK, OBTE_EPI_ROPE_QK, false>(GemmParams);
OBTE_INST3(true, true)
OBTE_INST3(true, false)
OBTE_INST3(false, true)
OBTE_INST3(false, false)
#undef OBTE_INST3
template __global__ void gemm_v3_kernel<false, false, OBTE_EPI_ACC32, false>(GemmParams);
template __global__ void gemm_v3_kernel<true, true, OBTE_EPI_GELU_ACT, false>(GemmParams);   // (x W^T only)

// ---- fourth structure: 256x128 tile, FOUR waves, ring of THREE half K-tiles (24 KiB each), TWO workgroups per CU ------------
// What the K = 1024 shapes of the block lose (measured with the timing-only hooks on c_fc + GELU, 8192 x 4096 x 1024: 96 us
// as it stands, 68 us without its stores, 52 us without loads and stores) is the store phase: with one workgroup per CU and
// one or two rounds of equal tiles every CU multiplies at the same time and then every CU stores at the same time — the
// matrix pipes idle while 134 MB drain at HBM rate.  A wave's own stores cannot hide under its own next tile either: vmcnt
// retires in issue order, so the first LDS-DMA wait behind a store burst waits for the burst.  The overlap has to come from a
// SECOND workgroup on the same CU.  This structure is the half-tile ring cut to fit twice: 4 waves x (64 x 128) output per
// wave (the same per-wave tile, fragments and MFMA interleave as the 256x256 structure), 256 threads, <= 256 VGPRs, 72 KiB of
// LDS (three half-stages, two of them in flight), so that two independent workgroups share each CU and each SIMD hosts one
// wave of either: their barriers, DMA waits and epilogues are unrelated and drift apart.
constexpr int V4_THREADS = 256;
constexpr int V4_BT = 128 * 32 * 2;             // 8 KiB: the B half tile (A: H_TILE = 16 KiB)
constexpr int V4_STAGE = H_TILE + V4_BT;        // 24 KiB
constexpr int V4_RING = 3 * V4_STAGE;           // 72 KiB
constexpr int V4_EPI = 4 * 64 * 272;            // epilogue staging of four 64 x 128 wave tiles
constexpr int V4_SMEM = V4_RING > V4_EPI ? V4_RING : V4_EPI;

// byte offsets of the LDS-DMA pieces (piece = wave + 4*i) of a half tile [MN rows][32 k] (k-contiguous) or [32 k][MN] (k-strided)
template <bool KMAJOR, int MN, int NP>
__device__ __forceinline__ void dma_offsets_v4(int wave, int lane, int64_t ld, int (&voff)[NP]) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int piece = wave + 4 * i;
        if (KMAJOR) {
            const int row = piece * 16 + (lane >> 2);
            const int chunk = (lane & 3) ^ ((4 - (row >> 2)) & 3);
            voff[i] = (int)((row * ld + chunk * 8) * 2);
        } else {
            constexpr int CPR = MN / 8;          // 16-B chunks per k-row: 32 (A) or 16 (B)
            constexpr int RPP = 64 / CPR;        // k-rows per 1-KiB piece: 2 or 4
            const int krow = piece * RPP + lane / CPR;
            const int chunk = (lane % CPR) ^ mn_f(krow);
            voff[i] = (int)((krow * ld + chunk * 8) * 2);
        }
    }
}
template <bool KMAJOR, int MN>
__device__ __forceinline__ bf16x8 load_frag_v4(const char* tile, int mn0, int lane) {
    if (KMAJOR) return *reinterpret_cast<const bf16x8*>(tile + kmaj32_off(mn0 + (lane & 15), lane >> 4));
    return load_frag<false, MN>(tile, mn0, 0, lane);
}

template <bool A_KMAJOR, bool B_KMAJOR, int EPI, bool SPLIT>
__global__ __launch_bounds__(V4_THREADS, 2) void gemm_v4_kernel(GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (p.store_rows < 0) return;
#ifdef OBTE_DEBUG_HOOKS
    if (p.delay_sleeps > 0 && blockIdx.x < 512) {   // first round only: HW_REG_HW_ID[3:0] = wave slot on the SIMD
        const unsigned hw = __builtin_amdgcn_s_getreg(0x1804);
        if (hw & 1) for (int i = 0; i < p.delay_sleeps; ++i) __builtin_amdgcn_s_sleep(127);
    }
#endif
    constexpr int NJ = 8;
    const int wgid = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n * p.splits);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int split = wgid % p.splits;
    const int tid_ = wgid / p.splits;
    const int group_sz = 8 * p.tiles_n;
    const int first_m = (tid_ / group_sz) * 8;
    const int gsz = min(p.tiles_m - first_m, 8);
    const int tm = first_m + (tid_ % group_sz) % gsz;
    const int tn = (tid_ % group_sz) / gsz;
    const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * 128;

    int voff_a[4], voff_b[2];
    dma_offsets_v4<A_KMAJOR, 256, 4>(wave, lane, p.lda, voff_a);
    dma_offsets_v4<B_KMAJOR, 128, 2>(wave, lane, p.ldb, voff_b);

    f32x4 acc[NJ][4];
#pragma unroll
    for (int i = 0; i < NJ; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk_total = (int)((p.K + BKT - 1) / BKT);
    const int kt0 = split * p.k_per_split;
    const int nh = 2 * min(p.k_per_split, nk_total - kt0);   // half-steps; even, >= 4 (checked by the host)

    // LDS-DMA of half-stage u into ring slot `slot`: pieces g = 0..3 of A and 0..1 of B for this wave
    auto dma_piece = [&](int u, int slot, int g) {
        const int64_t k0 = (int64_t)kt0 * BKT + (int64_t)u * 32;
        const int64_t ao = A_KMAJOR ? (m0 * p.lda + k0) : (k0 * p.lda + m0);
        const uint32_t lds_st = lds_addr_of(smem + slot * V4_STAGE) + wave * 1024;
        lds_dma16(make_rsrc_words(p.a + ao, (p.a_elems - ao) * 2), lds_st + 4 * g * 1024, voff_a[g]);
        if (g < 2) {
            const int64_t bo = B_KMAJOR ? (n0 * p.ldb + k0) : (k0 * p.ldb + n0);
            lds_dma16(make_rsrc_words(p.b + bo, (p.b_elems - bo) * 2), lds_st + H_TILE + 4 * g * 1024, voff_b[g]);
        }
    };
    auto issue = [&](int u, int slot) {
#pragma unroll
        for (int g = 0; g < 4; ++g) dma_piece(u, slot, g);
    };
    auto load_frags = [&](int slot, bf16x8 (&af)[4], bf16x8 (&bfr)[NJ]) {
        const char* ta = smem + slot * V4_STAGE;
        const char* tb = ta + H_TILE;
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = load_frag_v4<A_KMAJOR, 256>(ta, wave * 64 + i * 16, lane);
#pragma unroll
        for (int i = 0; i < NJ; ++i) bfr[i] = load_frag_v4<B_KMAJOR, 128>(tb, i * 16, lane);
    };
    auto mma = [&](const bf16x8 (&af)[4], const bf16x8 (&bfr)[NJ]) {
#pragma unroll
        for (int ni = 0; ni < NJ; ++ni)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[ni][mi], 0, 0, 0);
    };
    // half-step uu with F(uu) in (af, bfr): group g = {A fragment g and B fragments 2g, 2g+1 of half-step uu+1 from slot rs,
    // the LDS-DMA pieces g of half-step uu+3 into slot ds (= the slot of uu: every wave holds F(uu) in registers since the
    // barrier), the 8 MFMAs of n sub-tiles 2g, 2g+1}
    auto istep = [&](int uu, int rs, int ds, const bf16x8 (&af)[4], const bf16x8 (&bfr)[NJ], bf16x8 (&an)[4], bf16x8 (&bn)[NJ]) {
        const char* ta = smem + rs * V4_STAGE;
        const char* tb = ta + H_TILE;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            an[g] = load_frag_v4<A_KMAJOR, 256>(ta, wave * 64 + g * 16, lane);
            bn[2 * g] = load_frag_v4<B_KMAJOR, 128>(tb, (2 * g) * 16, lane);
            bn[2 * g + 1] = load_frag_v4<B_KMAJOR, 128>(tb, (2 * g + 1) * 16, lane);
            dma_piece(uu + 3, ds, g);
#pragma unroll
            for (int ni = 2 * g; ni < 2 * g + 2; ++ni)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[ni][mi], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    bf16x8 a0[4], b0[NJ], a1[4], b1[NJ];
    issue(0, 0); issue(1, 1); issue(2, 2);
    __builtin_amdgcn_s_waitcnt(0x007C);   // vmcnt(12): half-stage 0 landed (two stages of six pieces stay in flight)
    __builtin_amdgcn_s_barrier();
    load_frags(0, a0, b0);
    int u = 0;
    int s0 = 0, s1 = 1, s2 = 2;           // ring slots of half-steps u, u+1, u+2
    for (; u + 4 < nh; u += 2) {
        __builtin_amdgcn_s_waitcnt(0x0076);   // vmcnt(6) lgkmcnt(0): half-stage u+1 landed, F(u) reads complete
        __builtin_amdgcn_s_barrier();
        istep(u, s1, s0, a0, b0, a1, b1);      // DMA(u+3) -> slot of u
        __builtin_amdgcn_s_waitcnt(0x0076);
        __builtin_amdgcn_s_barrier();
        istep(u + 1, s2, s1, a1, b1, a0, b0);  // DMA(u+4) -> slot of u+1
        const int t = s0; s0 = s2; s2 = s1; s1 = t;   // slots of u+2, u+3 (= old s0), u+4 (= old s1)
    }
    // last four half-steps (u == nh - 4): half-stage u+3 is still to be issued, then the waits count down
    __builtin_amdgcn_s_waitcnt(0x0076);
    __builtin_amdgcn_s_barrier();
    istep(u, s1, s0, a0, b0, a1, b1);          // DMA(u+3) -> s0; F(u+1) -> (a1, b1)
    __builtin_amdgcn_s_waitcnt(0x0076);        // half-stage u+2 landed (u+3 in flight)
    __builtin_amdgcn_s_barrier();
    load_frags(s2, a0, b0);
    __builtin_amdgcn_sched_barrier(0);
    mma(a1, b1);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0x0070);        // vmcnt(0): half-stage u+3 landed
    __builtin_amdgcn_s_barrier();
    load_frags(s0, a1, b1);
    __builtin_amdgcn_sched_barrier(0);
    mma(a0, b0);
    mma(a1, b1);
    tile_epilogue<EPI, SPLIT, 256>(p, acc, smem, wave, lane, m0, n0, wave, 0, split, 128);   // the 64 x 128 wave tile of the 256-wide epilogue
}

#define OBTE_INST4(AK, BK)                                                                   \
    template __global__ void gemm_v4_kernel<AK, BK, OBTE_EPI_NONE, true>(GemmParams);        \
    template __global__ void gemm_v4_kernel<AK, BK, OBTE_EPI_NONE, false>(GemmParams);       \
    template __global__ void gemm_v4_kernel<AK, BK, OBTE_EPI_GELU, false>(GemmParams);       \
    template __global__ void gemm_v4_kernel<AK, BK, OBTE_EPI_ADD, false>(GemmParams);        \
    template __global__ void gemm_v4_kernel<AK, BK, OBTE_EPI_GELU_BWD, false>(GemmParams);   \
    template __global__ void gemm_v4_kernel<AK, BK, OBTE_EPI_ADD_DROPOUT, false>(GemmParams); \
    template __global__ void gemm_v4_kernel<AK, BK, OBTE_EPI_ROPE_QK, false>(GemmParams);
OBTE_INST4(true, true)
OBTE_INST4(true, false)
OBTE_INST4(false, true)
OBTE_INST4(false, false)
#undef OBTE_INST4
template __global__ void gemm_v4_kernel<false, false, OBTE_EPI_ACC32, false>(GemmParams);
template __global__ void gemm_v4_kernel<true, true, OBTE_EPI_GELU_ACT, false>(GemmParams);   // (x W^T only)

// d[m][n] = bf16(alpha * sum_s slab[s][m][n]) in split order
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ slab, bf16* __restrict__ d, const bf16* aux,
                                                             int64_t MN4, int64_t MN, int splits, float alpha) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < MN4; i += (int64_t)gridDim.x * 256) {
        f32x4 s = *reinterpret_cast<const f32x4*>(slab + i * 4);
        for (int k = 1; k < splits; ++k) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(slab + k * MN + i * 4);
            s += t;
        }
        bf16x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = f2bf(s[j] * alpha);
        if (aux) {   // EPI_ADD: d = bf16(aux + bf16(acc)); aux may alias d (each element is read, then written, by one thread)
            const bf16x4 r = *reinterpret_cast<const bf16x4*>(aux + i * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = f2bf(bf2f(r[j]) + bf2f(o[j]));
        }
        *reinterpret_cast<bf16x4*>(d + i * 4) = o;
    }
}

// OBTE_EPI_ACC32 after a split-K launch: c = fl32(alpha * sum_s slab[s][m][n]) in split order, acc32 (+)= c by mode, d = bf16(acc32) on LAST
__global__ __launch_bounds__(256) void splitk_reduce_acc32_kernel(const float* __restrict__ slab, float* __restrict__ acc32, bf16* __restrict__ d,
                                                                   int64_t MN4, int64_t MN, int splits, float alpha, int mode) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < MN4; i += (int64_t)gridDim.x * 256) {
        f32x4 s = *reinterpret_cast<const f32x4*>(slab + i * 4);
        for (int k = 1; k < splits; ++k) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(slab + k * MN + i * 4);
            s += t;
        }
        f32x4 v = acc32_term(s, alpha);
        if (mode != OBTE_ACC32_FIRST) v = acc32_sum(*reinterpret_cast<const f32x4*>(acc32 + i * 4), v);
        *reinterpret_cast<f32x4*>(acc32 + i * 4) = v;
        if (mode == OBTE_ACC32_LAST) *reinterpret_cast<bf16x4*>(d + i * 4) = __builtin_convertvector(v, bf16x4);
    }
}

}  // namespace obte_gemm_v2
using namespace obte_gemm_v2;

// ---- launchers (gemm_common.h) ---------------------------------------------------------------------------------------------------------
int obte_gemm_splitk_reduce(const GemmParams& p, const bf16* aux, hipStream_t st) {
    const int64_t mn = p.M * p.N;
    int64_t blocks = cdiv64(mn / 4, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)p.slab, p.d, aux, mn / 4, mn, p.splits, p.alpha);
    hipError_t e_ = hipGetLastError();
    if (e_ != hipSuccess) { obte_set_error("obte_gemm_bf16(split-K reduce): %s", hipGetErrorString(e_)); return OBTE_ELAUNCH; }
    return OBTE_OK;
}

int obte_gemm_splitk_reduce_acc32(const GemmParams& p, hipStream_t st) {
    const int64_t mn = p.M * p.N;
    int64_t blocks = cdiv64(mn / 4, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(splitk_reduce_acc32_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)p.slab, p.acc32, p.d, mn / 4, mn, p.splits, p.alpha,
                       p.acc32_mode);
    hipError_t e_ = hipGetLastError();
    if (e_ != hipSuccess) { obte_set_error("obte_gemm_bf16(split-K reduce, fp32 sum): %s", hipGetErrorString(e_)); return OBTE_ELAUNCH; }
    return OBTE_OK;
}

template <int BN>
int obte_gemm_v2_launch(const GemmParams& p, bool ak, bool bk, int epi, hipStream_t st) {
    return gemm_dispatch<2, BN>(ak, bk, epi, p.splits > 1, [&](auto f) {
        using F = decltype(f);
        return gemm_launch<gemm_v2_kernel<F::a_kmajor, F::b_kmajor, F::epilogue, F::split, BN>, Cfg<BN>::SMEM>(p.tiles_m * p.tiles_n * p.splits, NTHREADS, st, p);
    });
}
template int obte_gemm_v2_launch<128>(const GemmParams&, bool, bool, int, hipStream_t);
template int obte_gemm_v2_launch<192>(const GemmParams&, bool, bool, int, hipStream_t);
template int obte_gemm_v2_launch<256>(const GemmParams&, bool, bool, int, hipStream_t);

int obte_gemm_v3_launch(const GemmParams& p, bool ak, bool bk, int epi, hipStream_t st) {
    return gemm_dispatch<3, 256>(ak, bk, epi, p.splits > 1, [&](auto f) {
        using F = decltype(f);
        return gemm_launch<gemm_v3_kernel<F::a_kmajor, F::b_kmajor, F::epilogue, F::split>, V3_SMEM>(p.tiles_m * p.tiles_n * p.splits, NTHREADS, st, p);
    });
}

int obte_gemm_v4_launch(const GemmParams& p, bool ak, bool bk, int epi, hipStream_t st) {
    return gemm_dispatch<4, 128>(ak, bk, epi, p.splits > 1, [&](auto f) {
        using F = decltype(f);
        return gemm_launch<gemm_v4_kernel<F::a_kmajor, F::b_kmajor, F::epilogue, F::split>, V4_SMEM>(p.tiles_m * p.tiles_n * p.splits, V4_THREADS, st, p);
    });
}

int obte_gemm_group_launch(const GroupParams& gp, hipStream_t st) {
    return gemm_launch<gemm_v3_group_kernel, V3_SMEM>(gp.first_wg[GROUP_MAX], NTHREADS, st, gp, "obte_gemm_grouped_bf16");
}
