// conv 3x3 (pad 1) as Winograd F(2x2, 3x3) on the fp16 matrix cores with f16x3 products (two-way split of f16_split.h, fp32
// accuracy for inputs inside fp16's range): the default kernel of conv2 / conv3 forward and of both data gradients (the same
// kernel on the transposed / flipped taps).  Shapes it does not cover run on the bf16x6 fallbacks (conv_wino_bf16x6_kernel.h,
// bf16x6_kernels.h).
//
//   Y = A^T [ sum_cin (G g G^T) . (B^T d B) ] A     d: 4x4 input patch, g: 3x3 taps, Y: 2x2 outputs (= one pooling window)
//   per frequency f = 4 i + j of the transform one GEMM  M_f[tile][cout] = sum_cin V_f[tile][cin] U_f[cin][cout].
//
// ONE persistent 768-thread workgroup per CU with SPECIALISED waves -- 4 producers (input transform: VALU + LDS) and 8 consumers
// (matrix cores) -- so that on every SIMD one producer wave transforms the next 16-channel chunk while two consumer waves multiply
// the current one.
// Task = 32 tiles (8 tile rows x 4 tile columns; columns are numbered across the whole batch, g = image * TW + tx, so a task
// may straddle two images and no column is wasted) x 64 output channels (layers with 128: two tasks per block); a workgroup
// walks its tasks chunk by chunk, step s: producers chunk s, consumers chunk s - 1, ONE barrier per step.
// With a compacted task list (inference pad skip, Wino2Geo::ctab) a task holds up to two SEGMENTS instead, each a run of tile
// columns of one image: segment A in the first tile slots and an optional guest segment B of another image in the last ones, their
// patch columns disjoint.  The DMA sources every patch column from its own segment's image, validity and stores map slot ->
// segment -> (image, tile column); transform, LDS layout and MFMA sequence do not know about it.
//   producers     raw 18 x 10 pixel patches of a chunk arrive by LDS-DMA (global_load_lds_dwordx4: no VGPRs, asynchronous) into
//                 a three-slot ring, issued two steps ahead; rows above / below the image, the pad column of an odd-width map
//                 and tile columns past the batch are sourced from a zero page, so the transform needs selects only in the one
//                 task in ~12 that holds an image boundary column.  LDS image: pixel (lr, lc) at position lr * 11 + lc +
//                 ((lr >> 1) & 1), its four 16-byte channel groups XOR-swizzled by ((lr >> 2) & 1) << 1: the ds_read_b128
//                 lane groups (8 tiles x 2 channel groups) hit 16 different slots of the 256-byte bank line for every patch
//                 offset (brute-forced: devtools/kernel_ab/wino2_lds_layout.py) while a DMA piece still reads whole 64-byte
//                 pixels.  B^T d B, the two-way fp16 split (Vh, Vl' = residual * 2^11) and the ds_write_b64 into V[step & 1]
//                 follow.  The producers' LDS accesses are inline asm and the barrier is a bare s_barrier behind
//                 s_waitcnt lgkmcnt(0): hipcc orders every LDS access it can see behind ALL outstanding LDS-DMA (vmcnt(0)) and
//                 __syncthreads() drains vmcnt as well.
//   consumers     wave (i, n): transform row i (4 frequencies), channel slice 32 n..: 4 accumulators that live across all chunks
//                 (no per-chunk folding); V fragments from LDS (ds_read_b128, 1 KB runs), U fragments (2 x 16 B per lane) streamed
//                 from L2 one chunk ahead, two frequencies at a time and fenced (left alone hipcc sinks the loads to the end of
//                 the step and the next step starts with an L2 round trip).  THREE products per frequency and 16-deep step --
//                 Vl' Uh, Vh Ul', Vh (Uh 2^11) -- into one accumulator that is 2^11 too large and scaled back in the epilogue;
//                 Uh 2^11 is formed in registers, so the U stream that bounds the kernel carries two planes.
//   epilogue      column inverse transform in registers, row transform across the four consumer waves of a channel slice through
//                 a DEDICATED exchange area (each wave finishes one tile column: it receives 3 x 2 KB): a consumer writes its
//                 pieces right behind its last MFMAs, the step's one barrier publishes them, and the producers are transforming
//                 the next chunk meanwhile.  Then BN + ReLU + 2x2 max (the 2x2 outputs of a tile ARE the pooling window) or raw
//                 outputs (+ channel statistics, accumulated in registers over the workgroup's tasks: 4 blocks per workgroup).
// Weights: prep_conv_w_wino_f16x3 (below), wpb[plane][chunk * 16 + f][cout][16 ch], two fp16 planes, column j = 3 negated; the data
// gradients take prep_conv_wT_wino_f16x3.  Needs inputs inside fp16's range (activations: yes; gradients only under the loss scale
// of the backward).
// What bounds it (timing knock-outs and stamps, profiles/r04/bench_conv_wino2_f16x3.txt): the U fragments a step pulls through the
// CU's vector-memory path (a fragment serves ONE 32-tile accumulator: 64-tile tasks need 128 accumulator registers per consumer,
// more than a three-wave SIMD has) and the instruction count of the producers' step; the part runs at its power cap, the matrix
// products are the energy.  Numbers and the structures that came before: DESIGN.md section 4.
#pragma once
#include "conv_wino_bf16x6_kernel.h"   // (bf16x6_kernels.h / f16_split.h: vector types and the split)
#include "wino2_geo.h"

constexpr int W2_RS = 11;                                   // pixel positions per raw row (10 + skew)
constexpr int W2_NPOS = 18 * W2_RS;
constexpr int W2_RAW_PIECES = (W2_NPOS * 4 + 63) / 64;      // 13 DMA pieces of 1 KB
constexpr int W2_RAW_BYTES = W2_RAW_PIECES * 1024;          // 13,312
constexpr int W2_PLB = 16 * 1024;                           // bytes per V plane: [f][1 KB]
constexpr int W2_NRAW = 3;                                  // raw ring slots: a chunk's DMA pieces get two steps to land
// two V planes per buffer (32 KB, two buffers) + the raw ring + a DEDICATED 48 KB exchange area for the epilogue's row transform: 64 + 39 + 48 KB
constexpr int W2_V_BYTES = 2 * W2_PLB;
constexpr int W2_XCH_BYTES = 3 * W2_PLB;
constexpr int W2_LDS_BYTES = 2 * W2_V_BYTES + W2_NRAW * W2_RAW_BYTES + W2_XCH_BYTES;   // 154,624
constexpr int W2_THREADS = 768;                             // 4 producer waves + 8 consumer waves
constexpr int W2_PPW = (W2_RAW_PIECES + 3) / 4;             // DMA pieces per wave of group B

// (W2Div, w2_div_make: wino2_geo.h)
__device__ __forceinline__ int w2_div(int n, const W2Div& d) {
    const unsigned un = (unsigned)n;
    if (d.pow2) return (int)(un >> d.sh);
    const unsigned t = __umulhi(d.m, un);
    return (int)((t + ((un - t) >> 1)) >> d.sh);
}

// ---- weights: U = G g G^T (transform as in conv_wino_bf16x6_kernel.h) as f16x3 planes (f16_split.h) ------------------------------
// TWO fp16 planes per value, same layout: plane 0 = Uh = fp16(U), plane 1 = Ul' = fp16((U - Uh) * 2^11).  With the activations
// split into (Vh, Vl') the kernel accumulates Vl' Uh + Vh Ul' + Vh (Uh 2^11) = 2^11 V U into ONE accumulator (three MFMAs, no
// second accumulator: the consumers' registers are full) and the epilogue scales by 2^-11; Uh 2^11 is formed in registers by the
// consumer (four v_pk_mul_f16 per fragment: its VALU is idle, and the U stream is what bounds the kernel -- a third plane would be
// a third more of it).  Uh * 2^11 is exact for |U| < 32; larger transformed weights are clamped and flagged in the handle's status
// word (bit 3: SIR_EINVAL at the next sir_check_status) -- conv weights of this model are O(0.1).
__device__ __forceinline__ void split_w_f16x3(float u, unsigned short& p0, unsigned short& p1, unsigned int* status) {
    constexpr float LIM = 31.984375f;                       // 65504 / 2048
    if (status && !(fabsf(u) <= LIM)) __hip_atomic_fetch_or(status, SIR_STATUS_CONV_WEIGHT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    u = __builtin_fminf(__builtin_fmaxf(u, -LIM), LIM);
    const _Float16 hi = (_Float16)u;
    const _Float16 lo = (_Float16)((u - (float)hi) * H3_LO_SCALE);
    p0 = __builtin_bit_cast(unsigned short, hi);
    p1 = __builtin_bit_cast(unsigned short, lo);
}
__device__ __forceinline__ void prep_conv_w_wino_f16x3_elem(const float* __restrict__ w, unsigned short* __restrict__ wpb, int cin, int cout, int idx,
                                                            unsigned int* status) {
    const int total = cin * 16 * cout;
    if (idx >= total) return;
    const int e = idx & 15, co = (idx >> 4) % cout, g = (idx >> 4) / cout;
    const int ci = (g / 16) * 16 + e, f = g % 16, i = f >> 2, j = f & 3;
    const float* gk = w + ((size_t)co * cin + ci) * 9;
    const float Gm[4][3] = {{1.f, 0.f, 0.f}, {.5f, .5f, .5f}, {.5f, -.5f, .5f}, {0.f, 0.f, 1.f}};
    float u = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float t = 0.0f;
#pragma unroll
        for (int l = 0; l < 3; ++l) t = fmaf(gk[k * 3 + l], Gm[j][l], t);
        u = fmaf(Gm[i][k], t, u);
    }
    if (j == 3) u = -u;
    split_w_f16x3(u, wpb[idx], wpb[(size_t)total + idx], status);
}
#ifndef SIR_NO_STANDALONE_KERNELS
static __global__ void prep_conv_w_wino_f16x3_kernel(const float* __restrict__ w, unsigned short* __restrict__ wpb, int cin, int cout,
                                                     unsigned int* status) {
    prep_conv_w_wino_f16x3_elem(w, wpb, cin, cout, blockIdx.x * blockDim.x + threadIdx.x, status);
}
#endif
__device__ __forceinline__ void prep_conv_wT_wino_f16x3_elem(const float* __restrict__ w, unsigned short* __restrict__ wpb, int cin_f, int cout_f,
                                                             int idx, unsigned int* status) {
    const int total = cout_f * 16 * cin_f;
    if (idx >= total) return;
    const int e = idx & 15, cop = (idx >> 4) % cin_f, g = (idx >> 4) / cin_f;
    const int co_f = (g / 16) * 16 + e, f = g % 16, i = f >> 2, j = f & 3;
    const float* gk = w + ((size_t)co_f * cin_f + cop) * 9;
    const float Gm[4][3] = {{1.f, 0.f, 0.f}, {.5f, .5f, .5f}, {.5f, -.5f, .5f}, {0.f, 0.f, 1.f}};
    float u = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float t = 0.0f;
#pragma unroll
        for (int l = 0; l < 3; ++l) t = fmaf(gk[8 - (k * 3 + l)], Gm[j][l], t);
        u = fmaf(Gm[i][k], t, u);
    }
    if (j == 3) u = -u;
    split_w_f16x3(u, wpb[idx], wpb[(size_t)total + idx], status);
}
#ifndef SIR_NO_STANDALONE_KERNELS
static __global__ void prep_conv_wT_wino_f16x3_kernel(const float* __restrict__ w, unsigned short* __restrict__ wpb, int cin_f, int cout_f,
                                                       unsigned int* status) {
    prep_conv_wT_wino_f16x3_elem(w, wpb, cin_f, cout_f, blockIdx.x * blockDim.x + threadIdx.x, status);
}
#endif

// OUT_MODE 0: pooled NHWC (BN + ReLU + max), 1: pooled in the GRU layout [b][tx][co * Hp + ty] (+ its f16x2 planes through
// `stats`), 2: raw NHWC + channel statistics (float2 {sum, sum of squares} at stats[(workgroup * 4 + row wave) * COUT + co]), 3: raw NHWC
// ---- LDS access behind the compiler's back (producer waves) ---------------------------------------------------------------
// hipcc orders every LDS read / write it can see behind ALL outstanding LDS-DMA of the wave (s_waitcnt vmcnt(0): it cannot prove
// that the DMA target and the access do not alias) and w2_barrier() drains vmcnt as well.  The producers keep two chunks of
// DMA pieces in flight, so their raw-patch reads and V writes are inline asm (invisible to the waitcnt pass), the waits are counted
// by hand and the barrier is a bare s_barrier behind s_waitcnt lgkmcnt(0).
typedef float w2_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned w2_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void w2_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// four 16-byte reads at base + 64 j, no wait (the caller waits once for all rows)
__device__ __forceinline__ void w2_read_row(unsigned base, w2_f32x4& r0, w2_f32x4& r1, w2_f32x4& r2, w2_f32x4& r3) {
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:64\n\tds_read_b128 %2, %4 offset:128\n\tds_read_b128 %3, %4 offset:192"
                 : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3) : "v"(base) : "memory");
}
template <int OFF>
__device__ __forceinline__ void w2_write64(unsigned base, uint2 v) {
    const w2_u32x2 d = {v.x, v.y};
    asm volatile("ds_write_b64 %0, %1 offset:%2" :: "v"(base), "v"(d), "n"(OFF) : "memory");
}

// DBG (devtools/kernel_ab/bench_conv.hip only): s_memtime stamps of the first producer and the first consumer wave of workgroup 0
__device__ long long w2_dbg_stamps[2][32];
__device__ long long w2_dbg_fine[8][8];              // producer wave 0 of workgroup 0, steps 8..15: loop top, DMA issued, raw patches read, V written, DMA wait over, barrier passed
// RAGGED (OUT_MODE 0 / 1 with a compacted column list; un-padded batch inference, model_infer.hip): image b is geo.wtab[b] >> geo.wsh pixel
// columns wide.  Columns past that width are the image edge: the raw-patch DMA sources them from the zero page (no selects in the
// transform, and whatever the map holds there is never read), and pooled columns past half that width are not stored.
template <int CIN, int COUT, int OUT_MODE, int DBG = 0, int PRIO = 3, bool RAGGED = false>
__global__ __launch_bounds__(W2_THREADS, 3) void conv3x3_wino2_f16x3_kernel(
    const float* __restrict__ x, const unsigned short* __restrict__ wpb, const float* __restrict__ scale,
    const float* __restrict__ shift, float* __restrict__ out, Wino2Geo geo, float2* __restrict__ stats, const float* __restrict__ zeros) {
    constexpr int NCH = CIN / 16, G = NCH * 16, NCHO = COUT >= 64 ? COUT / 64 : 1;
    static_assert(CIN % 16 == 0 && (COUT % 64 == 0 || COUT == 32), "16-channel chunks; 64-channel tasks (32: the n = 1 consumer waves only keep the barriers)");
    static_assert(NCH >= 2, "a task's exchange pieces are read behind its closing barrier; the next task's are written >= one barrier later");
    extern __shared__ __attribute__((aligned(1024))) unsigned char w2s[];
    constexpr int VB = W2_V_BYTES;                                      // bytes per V buffer
    unsigned char* const vbuf = w2s;                                    // [2][2 planes][16 f][1 KB]
    unsigned char* const rawbuf = w2s + 2 * VB;                         // [3][13 KB]
    unsigned char* const xchbuf = rawbuf + W2_NRAW * W2_RAW_BYTES;      // [8 waves][3 pieces][2 KB]

    // the wave index as a SCALAR (readfirstlane): everything derived from it -- roles, rows, channel slices, weight addresses -- then
    // lives in SGPRs; derived from threadIdx alone hipcc keeps it all in vector registers (+40 VGPRs in the consumer loop: spills)
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool producer = wv < 4;
    const int H = geo.H, W = geo.W, TW = geo.TW, NG = geo.NG, RBN = geo.RBN;
    const int* const ctab = OUT_MODE <= 1 ? geo.ctab : nullptr;      // (compacted lists: inference forms only)
    const int NS = ctab ? RBN * ctab[0] : geo.NS;
    // Dealing is static, round-robin over the resident workgroups.  A unit is (spatial task, 64-channel half).  The inference forms of a
    // 128-channel layer (HALF_DEAL) deal whole spatial tasks (both halves back to back on one workgroup) for the NS / gridDim full rounds and
    // the HALVES of the remaining spatial tasks one by one, so that a remainder costs one task-time, not two.  The other forms deal
    // spatial tasks only (OUT_MODE 2: the statistics' summation order is part of the result).
    constexpr bool HALF_DEAL = OUT_MODE <= 1 && NCHO > 1;
    const int GD = (int)gridDim.x, bx = (int)blockIdx.x;
    const int nfull = HALF_DEAL ? NS / GD : 0;                          // full rounds of spatial tasks (HALF_DEAL only)
    const int nfull_t = nfull * NCHO;
    const int ntask = HALF_DEAL ? nfull_t + ((NS - nfull * GD) * NCHO - bx + GD - 1) / GD : ((NS - bx + GD - 1) / GD) * NCHO;
    if (ntask <= 0) return;
    const int nsteps = ntask * NCH;                                     // chunks of this workgroup; step s: producers chunk s, consumers chunk s - 1

    // task lt of this workgroup: segment A's first tile column g0 and its tile count na, the guest word bw (Wino2Geo::ctab; -1: no guest),
    // first tile row ty0, output-channel half ch, spatial task s
    auto task_geo = [&](int lt, int& g0, int& na, int& bw, int& ty0, int& ch, int& s) {
        if (HALF_DEAL && lt >= nfull_t) {
            const int r = bx + (lt - nfull_t) * GD;
            s = nfull * GD + r / NCHO;
            ch = r % NCHO;
        } else {
            s = bx + (lt / NCHO) * GD;
            ch = lt % NCHO;
        }
        const int cb = w2_div(s, geo.dRBN), rb = s - cb * RBN;
        // (both words in ONE 8-byte load: hipcc reads the list with vector loads and waits for each at once)
        const int2 tw = ctab ? reinterpret_cast<const int2*>(ctab)[1 + cb] : make_int2((4 * cb) << 2 | 3, -1);
        g0 = tw.x >> 2; na = 1 + (tw.x & 3); bw = RAGGED ? -1 : tw.y; ty0 = 8 * rb;
    };
    // guest word -> first tile slot (8: none, no slot or patch column reaches it), first tile column and tile count of segment B
    auto guest_geo = [&](int g0, int bw, int& sB, int& gB, int& nB) {
        const bool guest = bw >= 0;
        sB = guest ? 2 + ((bw >> 1) & 1) : 8; gB = guest ? bw >> 2 : g0; nB = guest ? 1 + (bw & 1) : 0;
    };
    // ---- raw-patch DMA: WHO issues it ------------------------------------------------------------------------------------------
    // The four producer waves (piece k = wave + 4 i, counted vmcnt waits in their loop) -- except in a 32-channel layer (the
    // conv2 data gradient), where the four consumer waves of the missing second channel slice have nothing to do but keep the barriers: they take
    // the DMA over, on the producers' own schedule (chunk s + 2 at the top of step s, landed by the end of step s + 1).  Stamps inside a producer's
    // step put the issue of its 3-4 LDS-DMA pieces at ~620 of ~3500 cycles (155 per piece) on the kernel's critical waves.  (Handing the pieces to
    // the WORKING consumers of the 64-channel forms was measured and lost 10 %: behind their MFMAs a chunk has one step instead of two to land,
    // and the in-order return puts it in front of their weight fragments -- profiles/r04/bench_conv_wino2_f16x3.txt.)
    constexpr bool IDLE_DMA = COUT < 64;
    constexpr int D_STRIDE = 4, D_PPW = (W2_RAW_PIECES + D_STRIDE - 1) / D_STRIDE;
    const int d_stride = D_STRIDE;
    const int d_rank = producer ? wv : ((wv - 4) >> 1);               // (the idle waves are 5, 7, 9, 11)
    // (the task-independent part of a piece's address -- raw row, column, channel group, "hole" positions of the padded image -- is computed
    // once; per task a piece then costs a clamp, one magic-number division and the bounds test instead of ~60 instructions)
    int pre_lr[D_PPW], pre_lc[D_PPW], pre_part[D_PPW];
#pragma unroll
    for (int ii = 0; ii < D_PPW; ++ii) {
        const int slot = 64 * (d_rank + d_stride * ii) + lane, pos = slot >> 2, sp = slot & 3;
        const int lr = pos / W2_RS;
        const int lc = pos - lr * W2_RS - ((lr >> 1) & 1);
        const bool hole = lr > 17 || lc < 0 || lc > 9;
        pre_lr[ii] = hole ? (1 << 20) : lr;                           // a hole fails the row test of every task
        pre_lc[ii] = lc;
        pre_part[ii] = (sp ^ (((lr >> 2) & 1) << 1)) * 4;
    }
    auto raw_offsets = [&](int g0, int bw, int ty0, unsigned (&off)[D_PPW]) {
        // pixel columns P of the flattened batch that may be read: all of it, or (compacted list) the own image of the lane's segment
        // only.  Patch columns >= 2 sB belong to the guest segment, whose tile slot sB sits at patch column 2 sB: a per-lane SELECT
        // of the segment's column origin and bounds (no branch: nothing here may wait on the DMA pieces in flight)
        int sB, gB, nB;
        guest_geo(g0, bw, sB, gB, nB);
        const int gimg = ctab ? w2_div(g0, geo.dTW) : 0, gimgB = ctab ? w2_div(gB, geo.dTW) : 0;
        const int ploA = ctab ? 2 * TW * gimg : 0, phiA = ctab ? ploA + (RAGGED ? min(W, geo.wtab[gimg] >> geo.wsh) : W) : 2 * NG;
        const int ploB = 2 * TW * gimgB, phiB = ploB + W;
        const int cA = 2 * g0 - 1, cB = 2 * (gB - sB) - 1, lcB = 2 * sB;
#pragma unroll
        for (int ii = 0; ii < D_PPW; ++ii) {
            const int gy = 2 * ty0 - 1 + pre_lr[ii];
            const bool inB = pre_lc[ii] >= lcB;
            const int plo = inB ? ploB : ploA, phi = inB ? phiB : phiA;
            const int P = (inB ? cB : cA) + pre_lc[ii];
            const int Pc = min(max(P, 0), 2 * NG - 1);
            const int bb = w2_div(Pc, geo.d2TW), px = Pc - bb * 2 * TW;
            const bool ok = gy >= 0 && gy < H && P >= plo && P < phi && px < W;
            off[ii] = ok ? (unsigned)(((bb * H + gy) * W + px) * CIN + pre_part[ii]) : ~0u;
        }
    };
        auto raw_issue = [&](const unsigned (&off)[D_PPW], int c, int slot_buf) {
#pragma unroll
        for (int ii = 0; ii < D_PPW; ++ii) {
            const int k = d_rank + d_stride * ii;
            if (k < W2_RAW_PIECES) {
                const float* src = off[ii] == ~0u ? zeros : x + off[ii];
                __builtin_amdgcn_global_load_lds((sir_gptr_t)(src + c * 16), (sir_lptr_t)(rawbuf + slot_buf * W2_RAW_BYTES + k * 1024), 16, 0, 0);
            }
        }
    };
    // chunk q (global index over this workgroup's tasks) -> issue its pieces into ring slot q % 3
    int ig0, ina, ibw, ity0, ich, is_;
    unsigned roff[D_PPW];
    int roff_task = -1;
    auto issue_chunk = [&](int q) {
        if (q >= nsteps) return;
        const int lt = q / NCH, c = q - lt * NCH;
        if (lt != roff_task) { task_geo(lt, ig0, ina, ibw, ity0, ich, is_); raw_offsets(ig0, ibw, ity0, roff); roff_task = lt; }
        raw_issue(roff, c, q % W2_NRAW);
    };
    int nst = 0;
    auto stamp = [&]() {
        if (DBG && blockIdx.x == 0 && lane == 0 && (wv == 0 || wv == 4) && nst < 32) w2_dbg_stamps[producer ? 0 : 1][nst] = __builtin_amdgcn_s_memtime();
        ++nst;
    };

    if (producer) {
        // ================= producers ==============================================================================================
        // (their VALU stream competes with two MFMA-issuing consumer waves for the SIMD's issue port: priority to the producer)
        if (PRIO) __builtin_amdgcn_s_setprio(PRIO);
        // MODE.FP16_OVFL = 1 for the producer waves: a conversion to fp16 that overflows gives +-65504 instead of infinity, which is what
        // the split's two v_med3 clamps per pair were for (32 of the ~170 vector instructions per row pair and step)
        __builtin_amdgcn_s_setreg((1 /* HW_REG_MODE */) | (23 << 6) | (0 << 11), 1);
        const int wg = wv;
        // wave wg = (row pair tR of the transform, 8-channel half tH); lane = (tile tm, 4-channel group tP1)
        const int tR = wg >> 1, tH = wg & 1, tm = lane >> 1, tP1 = lane & 1;
        const int tty = tm & 7, ttx = tm >> 3, tpart = 2 * tH + tP1;
        // DMA source of this lane's pieces for a task: element offset into x, or ~0u = the zero page (rows above / below the image,
        // the pad column of an odd-width map, tile columns past the batch: the transform then needs no selects for them)
        // loop-invariant LDS offsets of this thread: patch pixel (row rr, j = 0) inside a raw slot, its V destination inside a V buffer
        unsigned ra_rel[3];
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
            const int lr = 2 * tty + tR + rr;
            ra_rel[rr] = (unsigned)((lr * W2_RS + 2 * ttx + ((lr >> 1) & 1)) * 64 + ((tpart ^ (((lr >> 2) & 1) << 1)) * 16));
        }
        const unsigned raw_a = (unsigned)(uintptr_t)rawbuf, v_a = (unsigned)(uintptr_t)vbuf + (8 * tR) * 1024 + tH * 512 + tm * 16 + tP1 * 8;
        if (!IDLE_DMA) {
            issue_chunk(0);
            issue_chunk(1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        w2_barrier();                                                   // raw chunks 0 and 1 have landed
        bool edge = false, z0 = false, z3 = false;                      // the task holds an image boundary column; this thread's tile sits at one
        auto fine = [&](int s_, int k_) {
            if (DBG && blockIdx.x == 0 && lane == 0 && wv == 0 && s_ >= 8 && s_ < 16) w2_dbg_fine[s_ - 8][k_] = __builtin_amdgcn_s_memtime();
        };
#pragma unroll 1
        for (int s = 0; s <= nsteps; ++s) {
            stamp();
            fine(s, 0);
            if (s < nsteps) {
                if (!IDLE_DMA && !(DBG & 2)) issue_chunk(s + 2);        // into the slot chunk s - 1 left (its reads ended before the last barrier)
                fine(s, 1);
                if (s % NCH == 0 && !ctab) {                            // first chunk of a task: where are its image boundaries (none in a compacted list)
                    int cg0, cna, cbw, cty0, cch, cs;
                    task_geo(s / NCH, cg0, cna, cbw, cty0, cch, cs);
                    const int t0 = cg0 - w2_div(cg0, geo.dTW) * TW;     // tile column of the task's first column inside its image
                    edge = !ctab && (t0 == 0 || t0 + 3 >= TW - 1);    // (compacted: no neighbouring image in the patch)
                    const int txx = (t0 + ttx) - w2_div(t0 + ttx, geo.dTW) * TW;
                    z0 = txx == 0; z3 = txx == TW - 1;
                }
                const unsigned rb = raw_a + (s % W2_NRAW) * W2_RAW_BYTES, vd = v_a + (s & 1) * VB;
                if (!(DBG & 4)) {
                w2_f32x4 q[3][4];
#pragma unroll
                for (int rr = 0; rr < 3; ++rr) w2_read_row(rb + ra_rel[rr], q[rr][0], q[rr][1], q[rr][2], q[rr][3]);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                fine(s, 2);
                if (edge) {                                             // (one task in ~12: the halo column belongs to the neighbouring image)
                    // a real branch (the asm keeps hipcc from turning it into 24 selects on the common path).  SELECT zero, do not
                    // multiply by it: the halo column was loaded from the neighbouring clip, and 0 * Inf / NaN of a corrupt
                    // neighbour would leak into this clip's boundary columns (eval-mode samples are independent in the reference)
                    asm volatile("" ::: "memory");
                    const w2_f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int rr = 0; rr < 3; ++rr) { q[rr][0] = z0 ? zero4 : q[rr][0]; q[rr][3] = z3 ? zero4 : q[rr][3]; }
                }
                // patch rows tR .. tR + 2 (row pair 0: i = 0: d0 - d2, i = 1: d1 + d2; pair 1 (rows 1,2,3): i = 2: d2 - d1, i = 3: d1 - d3).
                // tR is wave-uniform: two straight-line copies under a branch (as one body hipcc computed both and selected: 32 v_cndmask)
                auto rows = [&](auto trc) {
                    constexpr int TR = decltype(trc)::value;
#pragma unroll
                    for (int il = 0; il < 2; ++il) {
                        w2_f32x4 R[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (TR == 0) R[j] = il == 0 ? q[0][j] - q[2][j] : q[1][j] + q[2][j];
                            else         R[j] = il == 0 ? q[1][j] - q[0][j] : q[0][j] - q[2][j];
                        }
                        const w2_f32x4 V[4] = {R[0] - R[2], R[1] + R[2], R[2] - R[1], R[1] - R[3]};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const unsigned d = vd + (4 * il + j) * 1024;
                            uint2 sh, sl;
                            split2h_pair_ovfl(V[j].x, V[j].y, sh.x, sl.x);
                            split2h_pair_ovfl(V[j].z, V[j].w, sh.y, sl.y);
                            w2_write64<0>(d, sh);
                            w2_write64<W2_PLB>(d, sl);
                        }
                    }
                };
                if (tR == 0) rows(std::integral_constant<int, 0>{});
                else rows(std::integral_constant<int, 1>{});
                if (DBG) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                fine(s, 3);
                }
                // chunk s + 1 (issued a step ago) must have landed before the barrier; the pieces of chunk s + 2, just issued, may still fly
                // (a wave issues 3 or 4 pieces per chunk: allowing its 3 newest operations to be outstanding is safe for both)
                if (!IDLE_DMA) {
                    if (s + 2 < nsteps) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(W2_RAW_PIECES / 4) : "memory");
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
            }
            stamp();
            fine(s, 4);
            w2_barrier();
            fine(s, 5);
        }
        return;
    }

    // ================= consumers ==================================================================================================
    // wave (n = cw & 1, i = cw >> 1): channel slice 32 n.., transform row i (frequencies 4 i .. 4 i + 3, 4 accumulators)
    const int cw = wv - 4, mn = cw & 1, mi = cw >> 1, m = lane & 31, h = lane >> 5;
    if (COUT < 64 && mn == 1) {                                         // a 32-channel layer has no second slice: join the barriers --
        if (IDLE_DMA) {                                                 // -- and feed the raw-patch ring in the producers' stead
            if (!(DBG & 2)) { issue_chunk(0); issue_chunk(1); }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            w2_barrier();                                               // raw chunks 0 and 1 have landed
#pragma unroll 1
            for (int s = 0; s <= nsteps; ++s) {
                if (s < nsteps) {
                    if (!(DBG & 2)) issue_chunk(s + 2);                 // into the slot chunk s - 1 left (its reads ended before the last barrier)
                    // chunk s + 1 (issued a step ago) must have landed before the barrier; the 3 or 4 pieces just issued may still fly
                    if (s + 2 < nsteps) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(W2_RAW_PIECES / 4) : "memory");
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                w2_barrier();
            }
            return;
        }
        w2_barrier();
        w2_barrier();
        for (int lt = 0; lt < ntask; ++lt)
            for (int c = 0; c < NCH; ++c) w2_barrier();
        return;
    }
    // U fragment address = uniform part (plane, frequency, channel block, slice: scalar registers) + this lane's 32-bit byte offset
    const unsigned wlane = (unsigned)((m * 2 + h) * 16);
    const unsigned char* const wbase = reinterpret_cast<const unsigned char*>(wpb) + (size_t)mn * 1024;
    constexpr int NPW = 2;                                              // weight planes
    uint4 wq[4][NPW];                                                   // U fragments of the wave's four frequencies, one chunk ahead
    auto load_w = [&](int gidx, int chh, uint4 (&q)[NPW]) {
#pragma unroll
        for (int p = 0; p < NPW; ++p)
            q[p] = *reinterpret_cast<const uint4*>(wbase + ((size_t)(p * G + gidx) * (COUT * 2) + (size_t)chh * 128) * 16 + wlane);
    };
    int g0, na, bw, ty0, ch, s_idx;
    task_geo(0, g0, na, bw, ty0, ch, s_idx);
#pragma unroll
    for (int j = 0; j < 4; ++j) load_w(4 * mi + j, ch, wq[j]);
    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    w2_barrier();                                                    // (pairs with the producers' "raw chunks 0 and 1 have landed")
    float run_s[NCHO], run_q[NCHO];                                    // OUT_MODE 2: channel statistics of this wave's outputs, per channel block, over ALL its tasks
#pragma unroll
    for (int k = 0; k < NCHO; ++k) { run_s[k] = 0.0f; run_q[k] = 0.0f; }

    stamp();
    stamp();
    w2_barrier();                                                       // step 0: the producers transform the first chunk
    // step s = lt * NCH + c + 1 multiplies chunk sc = s - 1.  Nested loops (tasks, chunks) rather than one step loop with a runtime
    // "task ends here" flag: with the epilogue inside the step loop hipcc kept its working set alive through the matrix steps and
    // spilled the weight ring into them (376-480 B of scratch per lane for 64 and 128 input channels)
#pragma unroll 1
    for (int lt = 0; lt < ntask; ++lt) {
        int g0n = g0, nan_ = na, bwn = bw, ty0n = ty0, chn = ch, sn = s_idx;
        if (lt + 1 < ntask) task_geo(lt + 1, g0n, nan_, bwn, ty0n, chn, sn);
#pragma unroll 1
        for (int c = 0; c < NCH; ++c) {
            stamp();
            const int sc = lt * NCH + c;
            const bool task_end = c == NCH - 1;
            const unsigned char* abase = vbuf + (sc & 1) * VB + h * 512 + m * 16 + (4 * mi) * 1024;
            const int gnxt = (task_end ? 0 : c + 1) * 16 + 4 * mi;
            // two frequencies at a time (two independent accumulator chains in flight), each pair followed AT ONCE by the loads of ITS
            // weights for the next chunk, fenced: left to itself hipcc sinks all twelve weight loads to the end of the step and the next
            // step starts with an L2 round trip
#pragma unroll
            for (int jp = 0; jp < 2; ++jp) {
                constexpr int NPA = 2;
                bf16x8 a[2][NPA], bq[2][3];
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
#pragma unroll
                    for (int p = 0; p < NPA; ++p)
                        a[jj][p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(abase + p * W2_PLB + (2 * jp + jj) * 1024));
                    // planes (Uh, Ul') -> fragments (Uh, Uh 2^11, Ul')
                    const f16x8 uh = __builtin_bit_cast(f16x8, wq[2 * jp + jj][0]);
                    bq[jj][0] = __builtin_bit_cast(bf16x8, uh);
                    bq[jj][1] = __builtin_bit_cast(bf16x8, uh * (_Float16)2048.0f);
                    bq[jj][2] = __builtin_bit_cast(bf16x8, wq[2 * jp + jj][1]);
                }
                if (DBG & 8) {
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
                        acc[2 * jp + jj][0] += __builtin_bit_cast(float4, a[jj][0]).x + __builtin_bit_cast(float4, a[jj][1]).y + __builtin_bit_cast(float4, a[jj][NPA - 1]).z +
                                               __builtin_bit_cast(float4, bq[jj][0]).x + __builtin_bit_cast(float4, bq[jj][1]).y + __builtin_bit_cast(float4, bq[jj][2]).z;
                } else {
                    // a: 0 = Vh, 1 = Vl'; bq: 0 = Uh, 1 = Uh 2^11, 2 = Ul' -- the two cross terms first, then the main one
                    constexpr int HA[3] = {1, 0, 0}, HB[3] = {0, 2, 1};
#pragma unroll
                    for (int t3 = 0; t3 < 3; ++t3)
#pragma unroll
                        for (int jj = 0; jj < 2; ++jj)
                            acc[2 * jp + jj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[jj][HA[t3]]),
                                                                                      __builtin_bit_cast(f16x8, bq[jj][HB[t3]]), acc[2 * jp + jj], 0, 0, 0);
                }
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) if (!(DBG & 64)) load_w(gnxt + 2 * jp + jj, task_end ? chn : ch, wq[2 * jp + jj]);
                __builtin_amdgcn_sched_barrier(0);
            }
            stamp();
            if (!task_end) w2_barrier();
        }
        if (DBG & 16) { w2_barrier(); if (acc[0][0] == 1234.5f && acc[1][1] + acc[2][2] + acc[3][3] == 4.0f) out[0] = 1.0f; }
        else {
            {
                // column inverse transform (U_{i3} is stored negated); finisher k = row index of slice mn completes accumulator registers
                // 4 k .. 4 k + 3 (tile column k, tile rows 4 h + e).  Piece (source i -> finisher k): W_i[b][4 k + e] as two float4 (b)
                float4* const xch = reinterpret_cast<float4*>(xchbuf);
                float own[2][4];
#pragma unroll
                for (int b = 0; b < 2; ++b) {                          // one b at a time: 16 live registers instead of 32 beside the accumulators
                    const f32x16 Wc = b == 0 ? acc[0] + acc[1] + acc[2] : acc[1] - acc[2] + acc[3];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (k == mi) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) own[b][e] = Wc[4 * k + e];
                        } else {
                            float4* dst = xch + (size_t)((mn * 4 + mi) * 3 + ((k - mi - 1) & 3)) * 128 + lane;
                            dst[b * 64] = make_float4(Wc[4 * k], Wc[4 * k + 1], Wc[4 * k + 2], Wc[4 * k + 3]);
                        }
                    }
                }
                w2_barrier();                                        // the pieces are in LDS (this IS the step's closing barrier -- the
                                                                     // producers are already on the next chunk, nobody parks)
                // Y[0][b] = (W0 + W1) + W2, Y[1][b] = (W1 - W2) - W3: always in THIS order, whichever row the finishing wave holds itself --
                // the tile column a clip lands on depends on its position in the batch, and a clip's logits must not (bit for bit)
                float Y[2][2][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int kk = (mi - i - 1) & 3;                   // piece index of source row i for this finisher (3: i is this wave itself)
                    const float4* src = xch + (size_t)((mn * 4 + i) * 3 + (kk < 3 ? kk : 0)) * 128 + lane;
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const float4 v = src[b * 64];
                        const float w[4] = {i == mi ? own[b][0] : v.x, i == mi ? own[b][1] : v.y, i == mi ? own[b][2] : v.z, i == mi ? own[b][3] : v.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if (i == 0) Y[0][b][e] = w[e];
                            else if (i <= 2) Y[0][b][e] += w[e];
                            if (i == 1) Y[1][b][e] = w[e];
                            else if (i >= 2) Y[1][b][e] -= w[e];
                        }
                    }
                }
                const int co = ch * 64 + mn * 32 + m;
                float ssum = 0.0f, ssq = 0.0f;
                float sc_ = 1.0f, sh_ = 0.0f;
                constexpr float DESC = H3_LO_INV;                      // the f16x3 accumulators are 2^11 too large (exact power of two)
                if (OUT_MODE <= 1) { sc_ = scale[co] * DESC; sh_ = shift[co]; }
                {
                    // tile slot mi -> segment -> (image, tile column).  Slots between the segments and past a segment's count hold
                    // garbage: not stored, not counted
                    int sB, gB, nB;
                    guest_geo(g0, bw, sB, gB, nB);
                    const bool inB = mi >= sB;
                    const int sfirst = inB ? gB : g0, sk = inB ? mi - sB : mi, scnt = inB ? nB : na;
                    const int gc = sfirst + sk, img0 = w2_div(sfirst, geo.dTW);
                    const int img = w2_div(gc, geo.dTW), tx = gc - img * TW;
                    const bool tvalid = sk < scnt && gc < (ctab ? (img0 + 1) * TW : NG);
                    // pooled columns of this image (RAGGED: of its own width; a segment's columns all belong to the image of its first)
                    const int wpi = RAGGED ? min(geo.Wp, geo.wtab[img0] >> (geo.wsh + 1)) : geo.Wp;
                    if (OUT_MODE <= 1) {
                        float pooled[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float v = 0.0f;
#pragma unroll
                            for (int a = 0; a < 2; ++a)
#pragma unroll
                                for (int b = 0; b < 2; ++b) v = fmaxf(v, fmaf(Y[a][b][e], sc_, sh_));
                            pooled[e] = v;
                        }
                        if (tvalid && tx < wpi) {
                            if (OUT_MODE == 0) {
#pragma unroll
                                for (int e = 0; e < 4; ++e)
                                    out[(((size_t)img * geo.Hp + ty0 + 4 * h + e) * geo.Wp + tx) * COUT + co] = pooled[e];
                            } else {
                                const size_t oidx = ((size_t)img * geo.Wp + tx) * (COUT * geo.Hp) + (size_t)co * geo.Hp + ty0 + 4 * h;
                                const float4 v4 = make_float4(pooled[0], pooled[1], pooled[2], pooled[3]);
                                *reinterpret_cast<float4*>(out + oidx) = v4;
                                if (stats) {           // f16x2 planes [2][B * Wp][COUT * Hp] (f16_split.h) of the following GEMM's A operand
                                    unsigned short* planes = reinterpret_cast<unsigned short*>(stats);
                                    const size_t plane = (size_t)geo.B * geo.Wp * (COUT * geo.Hp);
                                    uint2 hh, ll;
                                    split2h_quad(v4, hh, ll);
                                    *reinterpret_cast<uint2*>(planes + oidx) = hh;
                                    *reinterpret_cast<uint2*>(planes + plane + oidx) = ll;
                                }
                            }
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
#pragma unroll
                            for (int a = 0; a < 2; ++a)
#pragma unroll
                                for (int b = 0; b < 2; ++b) {
                                    const int gy = 2 * (ty0 + 4 * h + e) + a, gx = 2 * tx + b;
                                    if (tvalid && gx < W) {
                                        const float v = Y[a][b][e] * DESC;
                                        out[(((size_t)img * H + gy) * W + gx) * COUT + co] = v;
                                        ssum += v;
                                        ssq = fmaf(v, v, ssq);
                                    }
                                }
                    }
                }
                if (OUT_MODE == 2) {                                     // (kept in registers across the tasks: one partial per workgroup and row wave)
#pragma unroll
                    for (int k = 0; k < NCHO; ++k)
                        if (k == ch) { run_s[k] += ssum; run_q[k] += ssq; }
                }
            }
        }
        g0 = g0n; na = nan_; bw = bwn; ty0 = ty0n; ch = chn; s_idx = sn;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    }
    if (OUT_MODE == 2 && stats) {
        // statistics block (workgroup, row wave): 4 gridDim.x blocks of COUT channels in all (wino2_stat_blocks), fixed summation order
#pragma unroll
        for (int k = 0; k < NCHO; ++k) {
            float a = run_s[k], q = run_q[k];
            a += __shfl_xor(a, 32);
            q += __shfl_xor(q, 32);
            if (h == 0) stats[((size_t)blockIdx.x * 4 + mi) * COUT + k * 64 + mn * 32 + m] = make_float2(a, q);
        }
    }
}

// `g`: wino2_geo of the launch (model_shape.h keeps the model's).  The dynamic-LDS opt-in (W2_LDS_BYTES) is the caller's: the library's
// goes through sir_lds_opt_in at its launch sites (model_infer.hip / model_train_fwd.hip / model_train_bwd.hip).
// ctab (OUT_MODE 0 / 1 only): compacted task list in device memory (Wino2Geo::ctab), at most ncol_max tasks
// RAGGED: per-image widths wtab[b] >> wsh (see the kernel); needs ctab
template <int CIN, int COUT, int OUT_MODE, int DBG = 0, int PRIO = 3, bool RAGGED = false>
static inline hipError_t launch_conv_wino2(hipStream_t st, Wino2Geo g, const float* x, const unsigned short* wpb, const float* scale,
                                           const float* shift, float* out, float2* stats, const float* zeros, int max_wg = 256,
                                           const int* ctab = nullptr, int ncol_max = 0, const int* wtab = nullptr, int wsh = 0) {
    if (RAGGED && (!ctab || !wtab)) return hipErrorInvalidValue;
    g.wtab = wtab; g.wsh = wsh;
    if (ctab) {
        if (OUT_MODE > 1 || ncol_max < 1) return hipErrorInvalidValue;
        g.ctab = ctab;
        g.NS = g.RBN * ncol_max;                                    // (grid size only: the kernel reads the real count)
    }
    const int nwg = g.NS < max_wg ? g.NS : max_wg;
    hipLaunchKernelGGL((conv3x3_wino2_f16x3_kernel<CIN, COUT, OUT_MODE, DBG, PRIO, RAGGED>), dim3(nwg), dim3(W2_THREADS), W2_LDS_BYTES, st, x, wpb, scale, shift, out, g, stats, zeros);
    return hipGetLastError();
}
