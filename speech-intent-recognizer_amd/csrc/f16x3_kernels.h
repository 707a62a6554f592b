// fp32-accurate contractions on the fp16 matrix cores with a TWO-way split ("f16x3").
//
// bf16x6 (bf16x6_kernels.h) pays six matrix products and three operand planes (6 bytes) per fp32 product; at the part's
// power cap the time of a contraction is energy per product, so fewer products and fewer operand bytes are what shortens
// it.  An fp32 value x splits into two fp16 numbers
//     hi = fp16(x)  (round to nearest, 11 significant bits)         lo = fp16((x - hi) * 2^11)
// (x - hi is exact in fp32; the residual is scaled by 2^11 so that it sits in fp16's normal range wherever hi does and
// no bit is lost to fp16's narrow exponent).  hi + lo * 2^-11 carries 22-23 significant bits of x.  Of the four cross
// products three are kept:
//     x * y  ~  hi_x * hi_y  +  2^-11 (hi_x * lo_y + lo_x * hi_y)            (lo * lo, weight 2^-22, dropped)
// as three v_mfma_f32_32x32x16_f16 into TWO f32 accumulators -- one for hi * hi, one for the two cross terms, which are
// 2^11 too large and are folded in once at the end (acc0 + 2^-11 acc1) -- and two operand planes (4 bytes per value).
// Per 16-deep k step: 96 matrix-pipe cycles instead of 192, 4 instead of 6 bytes per operand value through L2 / LDS.
// Accuracy: operand representation 2^-23 relative (against exact for bf16x3), dropped term 2^-22 * |lo_x lo_y| <= 2^-24
// relative; measured against a float64 product on the real GRU projection operands in profiles/r04/ab_f16x3.txt.
// Range: fp16's, |x| < 65504 (the GRU inputs are BatchNorm + ReLU outputs and GRU states; weights are O(0.1)); values
// below 2^-14 keep an ABSOLUTE error of 2^-36.
#pragma once
#include "bf16x6_kernels.h"     // (includes f16_split.h: the two-way split itself)

// ------------------------------------------------------------------------------------------
// C[m][z*N + n] = sum_k A[m][k] * Bz[n][k] + biasz[n] with A, B given as f16x2 planes (same contract as the
// bf16x6 GEMM it replaced, devtools/kernel_ab/legacy_kernels.h, with two planes per operand): Ap [2][M][K], Bp0 / Bp1 [2][N][K] fp16.
// Tile 160 x 256, BK = 32 (64 bytes per row and plane), 8 waves, wave = 160 x 32 strip: five hi*hi and five cross accumulators
// (160 registers).  Stage = A [2][160][64 B] + B [2][256][64 B] = 53,248 B; NST = 3 stages (159,744 B, the whole LDS of a CU):
// a K tile is now 30 MFMAs per wave (960 cycles; two waves per SIMD: ~0.8 us) -- shorter than an L2 round trip under load, so
// a tile's LDS-DMA pieces are issued TWO tiles ahead and the wait in front of the tile barrier is a counted vmcnt that leaves
// the newest tile's pieces in flight.  hipcc orders every LDS read it can see behind ALL outstanding LDS-DMA of the wave
// (vmcnt(0)), so the fragment reads are inline asm (12 ds_read_b128 + their wait per 16-deep step) and the barrier is a bare
// s_barrier.  Swizzle as in the bf16x6 kernel: 16-byte chunk c of row r sits at chunk c ^ ((r >> 2) & 3), applied on the SOURCE
// address of the DMA.  NST = 2 is the bf16x6 kernel's schedule (vmcnt(0) per tile), kept for the A/B.
// KNOCK (devtools/kernel_ab/bench_gemm.hip): bit 0 = no staging, bit 2 = no MFMAs (timing only).
// ------------------------------------------------------------------------------------------
constexpr int H3_BM = 160, H3_BN = 256, H3_BK = 32;
constexpr int H3_APLANE = H3_BM * 64, H3_BPLANE = H3_BN * 64;          // 10,240 / 16,384
constexpr int H3_BOFF = 2 * H3_APLANE;                                  // 20,480
constexpr int H3_STAGE = H3_BOFF + 2 * H3_BPLANE;                       // 53,248
constexpr int H3_APIECES = 2 * H3_BM / 16, H3_PIECES = H3_APIECES + 2 * H3_BN / 16;   // 20, 52
constexpr int H3_PPW = (H3_PIECES + 7) / 8;                             // 7 (waves 0-3: 7 pieces, waves 4-7: 6)
constexpr int h3_lds_bytes(int nst) { return nst * H3_STAGE; }

// A tile of BM = 96 / 128 / 160 rows (3 / 4 / 5 fragments of 32 rows per wave; the same 8 waves of 32-column strips, the same
// B tile, K order and MFMA sequence per output element, so every BM gives bit-identical results).  The stage holds A [2][BM][64 B]
// then B [2][256][64 B]; piece g < APIECES is A rows 16 (g % (BM / 16)).. of plane g / (BM / 16).
template <int BM>
struct H3Geo {
    static_assert(BM == 96 || BM == 128 || BM == 160, "BM = 96, 128 or 160");
    static constexpr int FR = BM / 32, ARG = BM / 16;
    static constexpr int APLANE = BM * 64, BOFF = 2 * APLANE, STAGE = BOFF + 2 * H3_BPLANE;
    static constexpr int APIECES = 2 * ARG, PIECES = APIECES + 2 * H3_BN / 16;
    static constexpr int PPW = (PIECES + 7) / 8, PREM = PIECES & 7;     // pieces of waves 0..PREM-1 (all if PREM = 0); the others one fewer
    static constexpr int ISTRIDE = 3 * FR / PPW;                        // a piece goes out after every ISTRIDE-th MFMA of the issuing step
};
static_assert(H3Geo<H3_BM>::STAGE == H3_STAGE && H3Geo<H3_BM>::PIECES == H3_PIECES && H3Geo<H3_BM>::PPW == H3_PPW, "160-row geometry");

// FR A fragments of one plane pair + the wave's B fragments of one 16-deep step, then the wait: 2 FR + 2 x ds_read_b128
// (offsets: A lo plane at APLANE, B hi at BOFF, B lo at BOFF + 16384 bytes)
template <int FR>
__device__ __forceinline__ void h3_read_step(unsigned aaddr, unsigned baddr, f16x8 (&ah)[FR], f16x8 (&al)[FR], f16x8& bh, f16x8& bl) {
    if constexpr (FR == 5) {
        asm volatile(
            "ds_read_b128 %0, %12\n\t"
            "ds_read_b128 %10, %13 offset:20480\n\t"
            "ds_read_b128 %5, %12 offset:10240\n\t"
            "ds_read_b128 %11, %13 offset:36864\n\t"
            "ds_read_b128 %1, %12 offset:2048\n\t"
            "ds_read_b128 %6, %12 offset:12288\n\t"
            "ds_read_b128 %2, %12 offset:4096\n\t"
            "ds_read_b128 %7, %12 offset:14336\n\t"
            "ds_read_b128 %3, %12 offset:6144\n\t"
            "ds_read_b128 %8, %12 offset:16384\n\t"
            "ds_read_b128 %4, %12 offset:8192\n\t"
            "ds_read_b128 %9, %12 offset:18432\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(ah[0]), "=&v"(ah[1]), "=&v"(ah[2]), "=&v"(ah[3]), "=&v"(ah[4]),
              "=&v"(al[0]), "=&v"(al[1]), "=&v"(al[2]), "=&v"(al[3]), "=&v"(al[4]), "=&v"(bh), "=&v"(bl)
            : "v"(aaddr), "v"(baddr)
            : "memory");
    } else if constexpr (FR == 4) {
        asm volatile(
            "ds_read_b128 %0, %10\n\t"
            "ds_read_b128 %8, %11 offset:16384\n\t"
            "ds_read_b128 %4, %10 offset:8192\n\t"
            "ds_read_b128 %9, %11 offset:32768\n\t"
            "ds_read_b128 %1, %10 offset:2048\n\t"
            "ds_read_b128 %5, %10 offset:10240\n\t"
            "ds_read_b128 %2, %10 offset:4096\n\t"
            "ds_read_b128 %6, %10 offset:12288\n\t"
            "ds_read_b128 %3, %10 offset:6144\n\t"
            "ds_read_b128 %7, %10 offset:14336\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(ah[0]), "=&v"(ah[1]), "=&v"(ah[2]), "=&v"(ah[3]),
              "=&v"(al[0]), "=&v"(al[1]), "=&v"(al[2]), "=&v"(al[3]), "=&v"(bh), "=&v"(bl)
            : "v"(aaddr), "v"(baddr)
            : "memory");
    } else {
        static_assert(FR == 3, "3, 4 or 5 fragments");
        asm volatile(
            "ds_read_b128 %0, %8\n\t"
            "ds_read_b128 %6, %9 offset:12288\n\t"
            "ds_read_b128 %3, %8 offset:6144\n\t"
            "ds_read_b128 %7, %9 offset:28672\n\t"
            "ds_read_b128 %1, %8 offset:2048\n\t"
            "ds_read_b128 %4, %8 offset:8192\n\t"
            "ds_read_b128 %2, %8 offset:4096\n\t"
            "ds_read_b128 %5, %8 offset:10240\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(ah[0]), "=&v"(ah[1]), "=&v"(ah[2]), "=&v"(al[0]), "=&v"(al[1]), "=&v"(al[2]), "=&v"(bh), "=&v"(bl)
            : "v"(aaddr), "v"(baddr)
            : "memory");
    }
}

// One (BM x 256) output tile `wgid` of C = A x [B0; B1]^T.  A's planes hold MA rows.  Dense (GATHER = false): output rows are A
// rows 0..M-1.  GATHER: output row i < M is A / C row rows[i] (a row list; model_infer.hip), and `rtab` is 512 ints of LDS.
template <int NST, int KNOCK, int BM, bool GATHER>
__device__ __forceinline__ void h3_gemm_tile(
    const unsigned short* __restrict__ Ap, const unsigned short* __restrict__ Bp0, const unsigned short* __restrict__ Bp1,
    const float* __restrict__ bias0, const float* __restrict__ bias1, float* __restrict__ C, int ldc, int M, int MA, int N, int K,
    int wgid, const int* __restrict__ rows, int* rtab) {
    static_assert(NST == 2 || NST == 3, "two or three stages");
    using G = H3Geo<BM>;
    constexpr int FR = G::FR, PPW = G::PPW;
    extern __shared__ __attribute__((aligned(1024))) unsigned char h3_smem[];
    const int nbd = N / H3_BN, nb = 2 * nbd;
    const int mblk = wgid / nb, nbk = wgid - mblk * nb, z = nbk / nbd;
    const int m0 = mblk * BM, n0 = (nbk - z * nbd) * H3_BN;
    const unsigned short* __restrict__ Bp = z ? Bp1 : Bp0;
    const float* __restrict__ bias = z ? bias1 : bias0;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), m = lane & 31, h = lane >> 5;
    const size_t planeA = (size_t)MA * K, planeB = (size_t)N * K;

    // LDS-DMA pieces of this wave: g = wv + 8 i; pieces 0..APIECES-1 = A (plane g / ARG, rows 16 (g % ARG)..), then B (plane
    // (g - APIECES) / 16, rows 16 ((g - APIECES) % 16)..); piece g lands at byte g * 1024 of its stage
    const int lr = lane >> 2;
    const int csrc = (lane & 3) ^ ((lr >> 2) & 3);
    // A row of piece i (clamped to the last row; GATHER: looked up in the list, every lookup issued before the first is waited for)
    constexpr int AI = (G::APIECES + 7) / 8;                // pieces i < AI can be A pieces
    int arow[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int g = wv + 8 * i < G::APIECES ? wv + 8 * i : 0;
        const int row = m0 + (g % G::ARG) * 16 + lr;
        arow[i] = row < M ? row : M - 1;
    }
    int orow = 0;
    if (GATHER) {
        const int ro = m0 + tid < M ? m0 + tid : M - 1;
        orow = rows[ro];
#pragma unroll
        for (int i = 0; i < AI; ++i) arow[i] = rows[arow[i]];
    }
    unsigned int poff[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int g = wv + 8 * i;
        const int gb = g - G::APIECES, pl = (gb >> 4) & 1, rg = gb & 15;
        if (GATHER) {                                       // both offsets, then a select: a lookup consumed on one side of a branch
            const unsigned pa = i < AI ? (unsigned)((g < G::APIECES ? g / G::ARG : 0) * planeA + (size_t)arow[i < AI ? i : 0] * K + csrc * 8) : 0u;
            const unsigned pb = (unsigned)(pl * planeB + (size_t)(n0 + rg * 16 + lr) * K + csrc * 8);
            poff[i] = g < G::APIECES ? pa : pb;             // only made hipcc wait for the prologue's LDS-DMA before reusing its register
        } else if (g < G::APIECES) {
            poff[i] = (unsigned int)(g / G::ARG * planeA + (size_t)arow[i < AI ? i : 0] * K + csrc * 8);
        } else {
            poff[i] = (unsigned int)(pl * planeB + (size_t)(n0 + rg * 16 + lr) * K + csrc * 8);
        }
    }
    // GATHER: the tile's output rows for the epilogue (orow, loaded beside the A rows above).  Rows past the list are clamped like
    // their A rows: they compute row M - 1's A row, so they store the very bits of output row M - 1 to its own C row again, and the
    // epilogue needs no branch (a branch per store made hipcc wait for every earlier store at each join).  No barrier of its own:
    // every wave's LDS writes have completed at its first h3_read_step (lgkmcnt(0)), before the barrier of K tile 1 (K >= 2 BK)
    if (GATHER) rtab[tid] = orow;                           // (all 512 threads: an unconditional store consumes every lookup)
    auto piece = [&](int i, int kt, int buf) {
        if (KNOCK & 1) return;
        const int g = wv + 8 * i;
        if (g < G::PIECES) {
            const unsigned short* src = (g < G::APIECES ? Ap : Bp) + poff[i] + (size_t)kt * H3_BK;
            __builtin_amdgcn_global_load_lds((sir_gptr_t)src, (sir_lptr_t)(h3_smem + buf * G::STAGE + g * 1024), 16, 0, 0);
        }
    };

    f32x16 acc0[FR], acc1[FR];
#pragma unroll
    for (int mt = 0; mt < FR; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[mt][r] = 0.0f; acc1[mt][r] = 0.0f; }

    // LDS byte address of this lane's chunk inside its row, per 16-deep step (stage 0)
    const unsigned sbase = (unsigned)(uintptr_t)h3_smem;
    unsigned fa[2], fb[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        fa[ks] = sbase + m * 64 + ((((ks << 1) | h) ^ ((m >> 2) & 3)) << 4);
        fb[ks] = fa[ks] + wv * 2048;
    }
    const int nk = K / H3_BK;

    // ISSUE: tile `ktn` (< nk) is staged into `bufn` between the MFMAs: waves 0-3 during step 0, their SIMD partners 4-7 during step 1
    auto compute = [&](int buf, auto issue_c, int ktn, int bufn) {
        constexpr bool ISSUE = decltype(issue_c)::value;
        const unsigned so = (unsigned)(buf * G::STAGE);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            f16x8 ah[FR], al[FR], bh, bl;
            h3_read_step<FR>(fa[ks] + so, fb[ks] + so, ah, al, bh, bl);
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int mt = 0; mt < FR; ++mt) {
                    if (KNOCK & 4) {
                        acc0[mt][0] += (float)ah[mt][0] * (float)bh[0] + (float)al[mt][1] * (float)bl[1];
                    } else {
                        if (t == 0) acc1[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mt], bh, acc1[mt], 0, 0, 0);
                        if (t == 1) acc1[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], bl, acc1[mt], 0, 0, 0);
                        if (t == 2) acc0[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], bh, acc0[mt], 0, 0, 0);
                    }
                    const int idx = t * FR + mt;
                    if (ISSUE && idx % G::ISTRIDE == G::ISTRIDE - 1 && idx / G::ISTRIDE < PPW && ks == (wv >> 2))
                        piece(idx / G::ISTRIDE, ktn, bufn);
                }
            __builtin_amdgcn_sched_barrier(0);              // (left alone hipcc sinks this step's MFMAs below the next step's reads: both fragment sets live, spills)
        }
    };

    // prologue: NST - 1 tiles in flight
#pragma unroll
    for (int s = 0; s < NST - 1; ++s)
        if (s < nk) {
#pragma unroll
            for (int i = 0; i < PPW; ++i) piece(i, s, s);
        }
    // tile kt must have landed before its barrier; the pieces of the tiles behind it (NST = 3: tile kt + 1, issued during the previous
    // tile) may still fly.  Main loop (stages the tile NST - 1 ahead) and tail (nothing left to stage) are two loops, not two branches
    // of one: with both bodies under one loop hipcc accumulated out of place (twice the accumulator registers, 290 spilled)
    auto tile_wait = [&](bool more) {
        if (NST == 2 || !more) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (G::PREM == 0 || wv < G::PREM) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PPW - 1) : "memory");
        asm volatile("s_barrier" ::: "memory");             // every wave's pieces of the tile are in LDS; the stage of the tile before it is free
    };
    int buf = 0, bufn = NST - 1, kt = 0;
    for (; kt + NST - 1 < nk; ++kt) {
        tile_wait(true);
        compute(buf, std::true_type{}, kt + NST - 1, bufn);
        buf = buf + 1 == NST ? 0 : buf + 1;
        bufn = bufn + 1 == NST ? 0 : bufn + 1;
    }
    for (; kt < nk; ++kt) {
        tile_wait(kt + 1 < nk);
        compute(buf, std::false_type{}, 0, 0);
        buf = buf + 1 == NST ? 0 : buf + 1;
    }

    const int n = n0 + wv * 32 + m;
    const float bv = bias ? bias[n] : 0.0f;
    if (GATHER) {                                           // each output row to its listed row (32-bit offsets: the launcher checks MA * ldc)
        float* cz = C + (size_t)z * N + n;
#pragma unroll
        for (int mt = 0; mt < FR; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int4 g4 = *reinterpret_cast<const int4*>(rtab + mt * 32 + 8 * i + 4 * h);
                const int gr[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) cz[gr[j] * ldc] = fmaf(acc1[mt][4 * i + j], H3_LO_INV, acc0[mt][4 * i + j]) + bv;
            }
        return;
    }
    float* crow = C + (size_t)(m0 + 4 * h) * ldc + (size_t)z * N + n;
    if (m0 + BM <= M) {                                     // whole tile in range: straight-line stores
#pragma unroll
        for (int mt = 0; mt < FR; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                crow[(size_t)(mt * 32 + (r & 3) + 8 * (r >> 2)) * ldc] = fmaf(acc1[mt][r], H3_LO_INV, acc0[mt][r]) + bv;
    } else {
#pragma unroll
        for (int mt = 0; mt < FR; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ro = mt * 32 + (r & 3) + 8 * (r >> 2);
                if (m0 + 4 * h + ro < M) crow[(size_t)ro * ldc] = fmaf(acc1[mt][r], H3_LO_INV, acc0[mt][r]) + bv;
            }
    }
}

// workgroup orig -> tile id: the hardware deals workgroups round-robin to the 8 XCDs (orig & 7); each XCD gets a contiguous range
// of the `nt` tile ids, so the N-blocks of one M-tile (which read the same A rows) share an L2
__device__ __forceinline__ int h3_xcd_tile(int orig, int nt) {
    const int xcd = orig & 7, q = nt >> 3, rem = nt & 7;
    return (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (orig >> 3);
}

template <int NST = 3, int KNOCK = 0>
static __global__ __launch_bounds__(512) void gemm_nt_f16x3_kernel(
    const unsigned short* __restrict__ Ap, const unsigned short* __restrict__ Bp0, const unsigned short* __restrict__ Bp1,
    const float* __restrict__ bias0, const float* __restrict__ bias1, float* __restrict__ C, int ldc, int M, int N, int K) {
    h3_gemm_tile<NST, KNOCK, H3_BM, false>(Ap, Bp0, Bp1, bias0, bias1, C, ldc, M, M, N, K, h3_xcd_tile(blockIdx.x, gridDim.x), nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------
// The same contraction over a ROW LIST (the inference pad skip, model_infer.hip): rows[0] = count, rows[1..count] = the A rows to
// compute, distinct and in ascending order; C row rows[1 + i] receives output row i, and every other C row is left alone.  A list
// of all MA rows is the identity: on the 160-row tile it runs the dense kernel's tile, without the lookups.  The list lives in
// device memory, so the grid is sized on the host for the worst case (count = MA) at the smallest tile, and each workgroup reads the
// real count and picks the tile (FBM: forced, for the harness) by one of two rules; workgroups past the real tile count exit before
// any barrier.  Tile ids are dealt to the XCDs over the REAL tile count.  Each output element sees the same MFMA sequence as in the
// dense kernel under every tile: the results are bit-identical to it.  LDS request: h3_lds_bytes(3) (the 160-row stages).
//
// LATENCY rule (h3_gather_bm; a launch that has the chip to itself): the SMALLEST of 96 / 128 / 160 rows whose tiles fit one
// workgroup per CU (ncu), else 160 -- an unpadded batch keeps the dense kernel's 160-row schedule and code.  It minimises the
// duration of the launch.
// THROUGHPUT rule (h3_gather_bm_throughput; launches that alternate between streams, sir_handle::cluster_multi): a workgroup holds
// a whole CU (full LDS), so while another stream's kernels want the CUs what counts is the CU time held, tiles x time per tile.
// The rule takes the tile that minimises ceil(count / bm) * cost(bm) (the smaller tile on a tie), cost = the measured time of one
// tile on a CU of its own (h3_gather_cost, 0.1 us; profiles/r10/README.md: MI355X, lib/bench_gemm gather, 3 353 listed rows):
//     K = 1024:  96 rows 40.2 us   128 rows 44.7 us   160 rows 51.3 us  (r06: 40.8 / 45.3 / 51.8)
//     K =  512:  96 rows 23.6 us   128 rows 26.1 us   160 rows 29.4 us  (the ragged path's layer-1 call)
// At the bench shape that is 126 workgroups of 160 rows, 6 464 workgroup-us, against 210 of 96 rows, 8 442 -- and 126 fit the 128
// CUs beside a GRU launch in one wave.  Pipelined step at batch 256: +2.6 to +3.4 % (r10), the 128-row tile forced: +1.2 %.
// FLOOR: CU time only matters when other work wants the CUs.  At or below H3_TP_FLOOR tiles of 96 rows the latency rule stays:
// pipelined over two streams (r10), the throughput rule loses 2 % at batch 128 per stream (1 689 rows, 108 tiles of 96 rows) and
// 4 % at batch 64 (54 tiles), ties at 32 and 16, and wins at 256 (210 tiles); the floor is the largest count at which it lost.
// ------------------------------------------------------------------------------------------
__host__ __device__ constexpr int h3_gather_tiles(int bm, int count, int N) { return (count + bm - 1) / bm * 2 * (N / H3_BN); }
__host__ __device__ constexpr int h3_gather_bm(int count, int N, int ncu) {
    return h3_gather_tiles(96, count, N) <= ncu ? 96 : h3_gather_tiles(128, count, N) <= ncu ? 128 : 160;
}
__host__ __device__ constexpr int h3_gather_cost(int bm, int K) {
    return K > 512 ? (bm == 96 ? 402 : bm == 128 ? 447 : 513) : (bm == 96 ? 236 : bm == 128 ? 261 : 294);
}
constexpr int H3_TP_FLOOR = 108;
__host__ __device__ constexpr int h3_gather_bm_throughput(int count, int N, int K, int ncu) {
    if (h3_gather_tiles(96, count, N) <= H3_TP_FLOOR) return h3_gather_bm(count, N, ncu);
    const int c96 = (count + 95) / 96 * h3_gather_cost(96, K), c128 = (count + 127) / 128 * h3_gather_cost(128, K),
              c160 = (count + 159) / 160 * h3_gather_cost(160, K);
    return c96 <= c128 && c96 <= c160 ? 96 : c128 <= c160 ? 128 : 160;
}

// `throughput`: the tile rule (above).  `rec` (optional, 2 ints): workgroup 0 leaves the row count it read and the tile it chose.
template <int KNOCK = 0, int FBM = 0>
static __global__ __launch_bounds__(512) void gemm_nt_f16x3_gather_kernel(
    const unsigned short* __restrict__ Ap, const unsigned short* __restrict__ Bp0, const unsigned short* __restrict__ Bp1,
    const float* __restrict__ bias0, const float* __restrict__ bias1, float* __restrict__ C, int ldc, const int* __restrict__ rows,
    int MA, int N, int K, int ncu, int throughput, int* __restrict__ rec) {
    __shared__ __attribute__((aligned(16))) int rtab[512];
    const int count = rows[0];
    const int bm = FBM ? FBM : throughput ? h3_gather_bm_throughput(count, N, K, ncu) : h3_gather_bm(count, N, ncu);
    const int nt = h3_gather_tiles(bm, count, N);
    if (blockIdx.x == 0 && threadIdx.x == 0 && rec) { rec[0] = count; rec[1] = bm; }
    if ((int)blockIdx.x >= nt) return;
    const int wgid = h3_xcd_tile(blockIdx.x, nt);
    if (bm == 96) h3_gemm_tile<3, KNOCK, 96, true>(Ap, Bp0, Bp1, bias0, bias1, C, ldc, count, MA, N, K, wgid, rows + 1, rtab);
    else if (bm == 128) h3_gemm_tile<3, KNOCK, 128, true>(Ap, Bp0, Bp1, bias0, bias1, C, ldc, count, MA, N, K, wgid, rows + 1, rtab);
    else if (count < MA) h3_gemm_tile<3, KNOCK, 160, true>(Ap, Bp0, Bp1, bias0, bias1, C, ldc, count, MA, N, K, wgid, rows + 1, rtab);
    else h3_gemm_tile<3, KNOCK, 160, false>(Ap, Bp0, Bp1, bias0, bias1, C, ldc, MA, MA, N, K, wgid, nullptr, nullptr);   // every row: the dense tile
}

static inline bool gemm_f16x3_ok(int M, int N, int K) {
    return N % H3_BN == 0 && K % H3_BK == 0 && (size_t)2 * M * K < ((size_t)1 << 31) && (size_t)2 * N * K < ((size_t)1 << 31);
}

// C[M][2 N] (+ bias) = A x [B0; B1]^T from pre-split f16x2 planes (the GRU input projections: N = 768 per direction)
static inline int launch_gemm_nt_f16x3(sir_handle* h, hipStream_t st, const unsigned short* Ap, const unsigned short* Bp0,
                                              const unsigned short* Bp1, const float* bias0, const float* bias1, float* C, int ldc,
                                              int M, int N, int K) {
    SIR_HIP_TRY(gemm_f16x3_ok(M, N, K) ? hipSuccess : hipErrorInvalidValue);
    SIR_TRY(sir_lds_opt_in(h, (const void*)gemm_nt_f16x3_kernel<3, 0>, h3_lds_bytes(3)));
    const int nwg = ((M + H3_BM - 1) / H3_BM) * 2 * (N / H3_BN);
    hipLaunchKernelGGL((gemm_nt_f16x3_kernel<3, 0>), dim3(nwg), dim3(512), h3_lds_bytes(3), st, Ap, Bp0, Bp1, bias0, bias1, C, ldc, M, N, K);
    SIR_KCHECK();
    return SIR_OK;
}

// the same over the row list `rows` (device memory: rows[0] = count <= MA, then the rows) of A's MA-row planes; no host sync.
// `throughput`: the tile rule for launches that share the chip with another stream's (above); `rec`: 2 ints or nullptr
static inline int launch_gemm_nt_f16x3_gather(sir_handle* h, hipStream_t st, const unsigned short* Ap, const unsigned short* Bp0,
                                                     const unsigned short* Bp1, const float* bias0, const float* bias1, float* C, int ldc,
                                                     const int* rows, int MA, int N, int K, bool throughput, int* rec) {
    // (K >= 2 BK: the K loop's barriers publish rtab)
    SIR_HIP_TRY(gemm_f16x3_ok(MA, N, K) && K >= 2 * H3_BK && (size_t)MA * ldc < ((size_t)1 << 31) ? hipSuccess : hipErrorInvalidValue);
    SIR_TRY(sir_lds_opt_in(h, (const void*)gemm_nt_f16x3_gather_kernel<0, 0>, h3_lds_bytes(3)));
    hipLaunchKernelGGL((gemm_nt_f16x3_gather_kernel<0, 0>), dim3(h3_gather_tiles(96, MA, N)), dim3(512), h3_lds_bytes(3), st, Ap, Bp0, Bp1,
                       bias0, bias1, C, ldc, rows, MA, N, K, h->num_cus, throughput ? 1 : 0, rec);
    SIR_KCHECK();
    return SIR_OK;
}
