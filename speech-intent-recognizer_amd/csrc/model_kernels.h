// Device kernels of the CNN + BiGRU + attention model (inference forms), gfx950.
// Included by model_infer.hip (and later by the training translation unit).
//
// Activation layout is channels-last ("NHWC") so that (a) conv outputs are stored as 128-byte
// runs of 32 consecutive channels per pixel and (b) the implicit-GEMM convolutions read their
// pixel-major A operand from LDS with one ds_read_b128 per four MFMA steps.
// All contractions use v_mfma_f32_32x32x2_f32 (f32 in / f32 accumulate, an exact fmaf chain:
// cdna guide section 3 "FP32-input MFMA") because the parity bar is identical argmax vs the fp32
// CPU path; lane maps: A[i=l&31][k=l>>5], B[k=l>>5][j=l&31], D col=l&31,
// row=(r&3)+8*(r>>2)+4*(l>>5).
#pragma once
#include "sir_internal.h"
#include "model_shape.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float mk_f32x2 __attribute__((ext_vector_type(2)));

#define SIR_BN_EPS 1e-5f
// SIR_NO_STANDALONE_KERNELS, defined by a translation unit in front of its includes: the non-template kernels of the shared headers
// (this one, f16_split.h, bf16x6_kernels.h, conv_wino_bf16x6_kernel.h, conv_wino2_f16x3_kernel.h) are left out.  A static __global__
// is compiled into every unit that sees it, launched there or not; a unit that only wants the device functions, templates and
// constants says so and the library holds no further copy.

// ------------------------------------------------------------------------------------------
// weight preparation (tiny, runs at the head of every forward so it always sees current weights)
// ------------------------------------------------------------------------------------------

// A conv1 weight or a BatchNorm weight / bias / statistic that is not finite sits in front of a ReLU and a max-pool that are fmaxf
// and drop a NaN: the kernels that fold these parameters raise bit 13 of the handle's status word instead (SIR_EINVAL at the next
// sir_check_status).
__device__ __forceinline__ bool sir_finite(float v) { return fabsf(v) < INFINITY; }
__device__ __forceinline__ void sir_flag_bn_param(bool ok, unsigned int* status) {
    if (!ok) __hip_atomic_fetch_or(status, SIR_STATUS_BN_PARAM, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// eval-mode BatchNorm folded to y = x*scale + shift (models/models.py:50-52, running stats).  w1 / n1: conv1's weights, looked at
// for non-finite values beside bn1's (NULL / 0 for the other blocks)
#ifndef SIR_NO_STANDALONE_KERNELS
static __global__ void prep_bn_kernel(const float* __restrict__ g, const float* __restrict__ b, const float* __restrict__ mean,
                               const float* __restrict__ var, float* __restrict__ scale, float* __restrict__ shift, int c,
                               const float* __restrict__ w1, int n1, unsigned int* __restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c) return;
    const float s = g[i] / sqrtf(var[i] + SIR_BN_EPS);
    const float t = b[i] - mean[i] * s;
    scale[i] = s;
    shift[i] = t;
    bool ok = sir_finite(s) && sir_finite(t);                // (a NaN or an infinity in any of the four reaches one of the two)
    for (int j = i; j < n1; j += c) ok = ok && sir_finite(w1[j]);
    sir_flag_bn_param(ok, status);
}
#endif

// ------------------------------------------------------------------------------------------
// conv1 (1 -> 32 channels) + BN + ReLU + 2x2 max-pool, direct form (K = 9: memory-bound)
//   x [B][H=64][W] -> out NHWC [B][H/2][W/2][32];  lane&31 = channel, half-waves walk pixels
// ------------------------------------------------------------------------------------------
constexpr int C1_PROWS = 4, C1_PCOLS = 32;          // pooled pixels per block: 4 x 32
constexpr int C1_TR = 2 * C1_PROWS + 2, C1_TC = 2 * C1_PCOLS + 2;
// launch grid of the MFMA kernels below: the image in x, the 32-column strip in z (see the body)
inline dim3 conv1_grid(int images, int Wp) { return dim3(images, 1, (Wp + C1_PCOLS - 1) / C1_PCOLS); }

// The same block on the f32 matrix pipe: the direct form above is bound by VALU issue (36 FMAs per output), and
// v_mfma_f32_32x32x2_f32 does 2048 of them per instruction at the packed-f32 vector rate while the VALU is free for the
// BN / ReLU / pooling epilogue.  GEMM view: D[channel i][pixel j] = sum_tap w[i][tap] x_tap[j], K = 9 taps padded to 10
// (five K = 2 steps; exact f32, an fmaf chain over the taps in order -- the same arithmetic as the direct form).
//   A operand (lane l): w[l & 31][2 s + (l >> 5)], five registers for the whole block;
//   B operand (lane l): tile[(row + ky) * C1_TC + col0 + (l & 31) + kx] for tap = 2 s + (l >> 5): one ds_read_b32;
//   D: lane l holds pixel l & 31, channels (r & 3) + 8 (r >> 2) + 4 (l >> 5), r = 0..15.
// Wave w = pooled row w of the 4 x 32 pooled-pixel block; per half (32 conv columns) two accumulators (the two conv rows
// of the pooled row); 2x2 max = max of the two accumulators and of lanes j, j ^ 1.  Even lanes then store channel groups
// 0, 1 and odd lanes groups 2, 3 of pooled pixel j / 2 (two float4 stores per lane).
// RAGGED (un-padded batch inference, model_infer.hip): frame columns >= xlim[b] of image b are the image edge -- read as zeros,
// whatever bits they hold -- and lim[b] = xlim[b] / 2 pooled columns are stored.
#ifndef SIR_NO_STANDALONE_KERNELS
template <bool RAGGED>
__device__ __forceinline__ void conv1_mfma_bn_relu_pool_body(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ scale,
    const float* __restrict__ shift, float* __restrict__ out, int H, int W, int Hp, int Wp,
    const float* __restrict__ xtail, int nx, const int* __restrict__ lim, const int* __restrict__ xlim) {
    // One block walks ALL row tiles of its column strip (grid = (B, 1, column strips)): weights / scale / shift are
    // loaded once, and the next tile's pixels are fetched into registers while the matrix pipe works on the current one
    // (one short block per tile spent most of its life waiting for its own loads: 50 us for 17 us of MFMA work).
    // The image is the FASTEST-varying part of the linear workgroup id, x + gridDim.x * (y + gridDim.y * z).  Under the pad
    // skip a strip is live (px0 < lim[b]) for some images and returns at once for the others; with the strip fastest, the live
    // ids of a batch of equal lengths were a fixed set of residues mod 8, and workgroups are dealt to the 8 XCDs round-robin by
    // id (observed, nothing relies on it but speed: see gru_quad_kernel), so at the bench shape -- 2 live strips of 4 -- half
    // the chip received only workgroups that exit.  Walking the images of one strip before the next strip begins makes the
    // live ids runs of consecutive numbers, whatever the lengths.
    // Inference pad skip (model_infer.hip): image b >= nx reads `xtail` instead of x (the all-zero template utterance), and
    // only pooled columns < lim[b] are computed and stored (lim == nullptr: all Wp).
    __shared__ float tiles[2][C1_TR * C1_TC];
    const int b = blockIdx.x, px0 = blockIdx.z * C1_PCOLS;
    const int wlim = lim ? min(Wp, lim[b]) : Wp;
    if (px0 >= wlim) return;                                 // (whole block, before any barrier)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, j = lane & 31, kh = lane >> 5;
    const float* xb = b < nx ? x + (size_t)b * H * W : xtail;
    const int Wx = RAGGED ? min(W, xlim[b]) : W;             // columns of this image that hold data
    constexpr int NPRE = (C1_TR * C1_TC + 255) / 256;
    float pre[NPRE];
    auto fetch = [&](int py0) {
#pragma unroll
        for (int q = 0; q < NPRE; ++q) {
            const int i = tid + 256 * q, ty = i / C1_TC, tx = i - ty * C1_TC;
            const int gy = 2 * py0 - 1 + ty, gx = 2 * px0 - 1 + tx;
            pre[q] = (i < C1_TR * C1_TC && gy >= 0 && gy < H && gx >= 0 && gx < Wx) ? xb[(size_t)gy * W + gx] : 0.0f;
        }
    };
    fetch(0);
    float wa[5];
    int boff[5];                                            // tile offset of this lane's tap in step s
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int tap = 2 * s + kh;
        wa[s] = tap < 9 ? w[j * 9 + tap] : 0.0f;            // j doubles as the channel index i of the A operand
        const int tc = tap < 9 ? tap : 8;
        boff[s] = (tc / 3) * C1_TC + (tc % 3) + j;
    }
    float sc[16], sh[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ch = (r & 3) + 8 * (r >> 2) + 4 * kh;
        sc[r] = scale[ch]; sh[r] = shift[ch];
    }
    const bool odd = j & 1;                                  // even lanes store channel groups 0, 1; odd lanes groups 2, 3
    int it = 0;
    for (int py0 = 0; py0 < Hp; py0 += C1_PROWS, ++it) {
        float* tile = tiles[it & 1];
#pragma unroll
        for (int q = 0; q < NPRE; ++q)
            if (tid + 256 * q < C1_TR * C1_TC) tile[tid + 256 * q] = pre[q];
        __syncthreads();                                     // (the other buffer was last read before the previous barrier)
        if (py0 + C1_PROWS < Hp) fetch(py0 + C1_PROWS);
        const int py = py0 + wv;
        if (py >= Hp) continue;
        const float* trow = tile + (2 * wv) * C1_TC;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (px0 + 16 * h >= wlim) break;                 // the last strip of a 100-column image has 4 valid columns
            f32x16 acc0, acc1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                const float b0 = trow[boff[s] + 32 * h], b1 = trow[boff[s] + 32 * h + C1_TC];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[s], b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[s], b1, acc1, 0, 0, 0);
            }
            float m[16];
            // BN of both conv rows as packed-f32 pairs (v_pk_fma_f32 / v_pk_max_f32: the same roundings, half the instructions -- the f32
            // MFMAs above run on the SAME ALUs as the vector f32 ops, so every instruction of this epilogue adds to the kernel's time)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const mk_f32x2 s2 = {sc[r], sc[r + 1]}, h2 = {sh[r], sh[r + 1]};
                const mk_f32x2 y0 = __builtin_elementwise_fma((mk_f32x2){acc0[r], acc0[r + 1]}, s2, h2);
                const mk_f32x2 y1 = __builtin_elementwise_fma((mk_f32x2){acc1[r], acc1[r + 1]}, s2, h2);
                // (scalar from here on: with the maximum taken on the pair, hipcc 7.2 expands the two DPP moves of its halves to TWO moves of
                // the SAME half -- element r + 1 then pooled against element r's neighbour)
                const float v0 = fmaxf(y0.x, y1.x), v1 = fmaxf(y0.y, y1.y);
                // neighbouring pixel = lane ^ 1: quad_perm(1, 0, 3, 2) on the DPP path (no LDS round trip)
                const float nb0 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v0), 0xB1, 0xF, 0xF, true));
                const float nb1 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v1), 0xB1, 0xF, 0xF, true));
                m[r] = fmaxf(fmaxf(v0, nb0), 0.0f);
                m[r + 1] = fmaxf(fmaxf(v1, nb1), 0.0f);
            }
            const int px = px0 + 16 * h + (j >> 1);
            const float4 lo = odd ? make_float4(m[8], m[9], m[10], m[11]) : make_float4(m[0], m[1], m[2], m[3]);
            const float4 hi = odd ? make_float4(m[12], m[13], m[14], m[15]) : make_float4(m[4], m[5], m[6], m[7]);
            if (px < wlim) {
                float* o = out + (((size_t)b * Hp + py) * Wp + px) * 32 + 4 * kh + (odd ? 16 : 0);
                *reinterpret_cast<float4*>(o) = lo;
                *reinterpret_cast<float4*>(o + 8) = hi;
            }
        }
    }
}
static __global__ __launch_bounds__(256, 4) void conv1_mfma_bn_relu_pool_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ scale,
    const float* __restrict__ shift, float* __restrict__ out, int H, int W, int Hp, int Wp,
    const float* __restrict__ xtail, int nx, const int* __restrict__ lim) {
    conv1_mfma_bn_relu_pool_body<false>(x, w, scale, shift, out, H, W, Hp, Wp, xtail, nx, lim, nullptr);
}
static __global__ __launch_bounds__(256, 4) void conv1_mfma_bn_relu_pool_ragged_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ scale,
    const float* __restrict__ shift, float* __restrict__ out, int H, int W, int Hp, int Wp,
    const int* __restrict__ lim, const int* __restrict__ xlim) {
    conv1_mfma_bn_relu_pool_body<true>(x, w, scale, shift, out, H, W, Hp, Wp, nullptr, (int)gridDim.x, lim, xlim);
}
#endif

// ------------------------------------------------------------------------------------------
// C[m][z*N + n] = sum_k A[m][k] * Bz[n][k] + biasz[n]    (fp32 MFMA, "NT": both operands k-contiguous)
//   used for the GRU input projections (z = direction) and the classifier head.
//   128 x 64 block tile, BK = 32, 4 waves as 2(M) x 2(N), wave tile 64 x 32; LDS rows padded to 36
//   floats so the ds_read_b128 operand reads are bank-conflict-free; global->register prefetch of
//   the next k-tile overlaps the MFMAs of the current one.
// ------------------------------------------------------------------------------------------
constexpr int GB_M = 128, GB_N = 64, GB_K = 32, GB_S = GB_K + 4;     // general (backward) GEMM tile

// ------------------------------------------------------------------------------------------
// GRU recurrence of one layer, both directions (torch.nn.GRU cell, gate order r,z,n, h0 = 0):
//   gi  [B*S][1536]   = x W_ih^T + b_ih for both directions (from the GEMM above)
//   wt  [2][64][768][4] transposed W_hh (prep_whh_kernel), bhh [2][768]
//   y   [B][S][512]   direction d writes columns d*256 .. d*256+255
// One workgroup = GRU_BW utterances of one direction for all S steps: no inter-workgroup traffic.
// 512 threads = 256 hidden units x 2 K-halves; a thread owns the 3 gate rows of its unit over
// its 128-wide K half.  W_hh is 786 KB per direction -- more than a CU can hold -- and
// re-streaming all of it from L2 every step is bound by the per-CU load path (round-1 profile:
// 7.5 us/step).  So 34 % of each thread's weights stay in REGISTERS and 12.5 % in LDS for all S
// steps (loaded once), and only the remaining 53 % is streamed per step as coalesced 16-byte
// loads, which the FMA work of the step now covers.  h is broadcast from LDS; the two K-halves are
// summed through LDS, then thread (u, b) applies the gate math for two utterances.
// SAVE: also store (r, z, n, W_hn h + b_hn) per step for back-propagation through time,
//   gates [B][S][2 dirs][4][256]
// ------------------------------------------------------------------------------------------
constexpr int GRU_H = 256, GRU_BW = 2;              // utterances per workgroup: 2 -> B/2 x 2 = 256 workgroups at B=256
constexpr int GRU_NPART = 4;                        // K split: threads = 256 units x NPART
constexpr int GRU_KPER4 = 64 / GRU_NPART;           // k/4 groups per part
constexpr int GRU_KREG4 = 3;                        // k/4 groups per part held in registers
constexpr int GRU_KLDS4 = 2;                        // ... held in LDS
constexpr int GRU_KSTR4 = GRU_KPER4 - GRU_KREG4 - GRU_KLDS4;   // ... streamed from L2 each step
constexpr int GRU_NQ = (GRU_BW + GRU_NPART - 1) / GRU_NPART;   // utterances finished per thread (bl = part + NPART*q)
constexpr int GRU_THREADS = 256 * GRU_NPART;
constexpr size_t GRU_LDS_BYTES =
    (size_t)(GRU_NPART * GRU_KLDS4 * 3 * 256 * 4 + GRU_BW * GRU_H + GRU_NPART * GRU_BW * 3 * GRU_H) * 4;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int NB>
__device__ __forceinline__ void gru_fma4(float (&acc)[NB], const float4 w, const float4 (&h4)[NB]) {
#pragma unroll
    for (int bb = 0; bb < NB; ++bb) {
        acc[bb] = fmaf(w.x, h4[bb].x, acc[bb]); acc[bb] = fmaf(w.y, h4[bb].y, acc[bb]);
        acc[bb] = fmaf(w.z, h4[bb].z, acc[bb]); acc[bb] = fmaf(w.w, h4[bb].w, acc[bb]);
    }
}

// ------------------------------------------------------------------------------------------
// attention pooling (models/models.py:63-64): scores = y a + b; softmax over time; ctx = sum_t w_t y_t
// one workgroup per utterance, wave shuffles for the 512-wide dots
// ------------------------------------------------------------------------------------------
// (ATT_MAX_S: model_shape.h)

// RAGGED (un-padded batch inference): utterance b has slen[b] <= SR steps in rows of stride SR; the softmax and the context sum run
// over those alone.  slen[b] = 0 marks an utterance whose length was rejected: its logits are NaN.
#ifndef SIR_NO_STANDALONE_KERNELS
template <bool RAGGED>
__device__ __forceinline__ void attention_pool_body(const float* __restrict__ y, const float* __restrict__ aw,
                                                    const float* __restrict__ ab, float* __restrict__ ctx,
                                                    int SR, const float* __restrict__ fcw,
                                                    const float* __restrict__ fcb, int C,
                                                    float* __restrict__ logits, long long* __restrict__ amax,
                                                    const int* __restrict__ slen, const int* __restrict__ bad_row,
                                                    const double* __restrict__ sumsq) {
    // fused tail (models.py:63-67 + evaluate.py:83): attention pooling, the 512 -> C classifier and the
    // arg-max of one utterance per workgroup.  The head is 31.7 kFLOP per utterance; as a separate
    // 128x64-tile MFMA GEMM it occupied 2 workgroups and cost 34 us per batch, fused here it is free.
    __shared__ float sc[ATT_MAX_S];
    __shared__ float cs[512];
    __shared__ float lg[64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int S = RAGGED ? min(SR, slen[b]) : SR;
    // a non-finite feature in this utterance (bad_row: pad_extent_kernel) or anywhere in a batch-normalised batch (sumsq: the sum of
    // the squared features) makes the row's logits NaN, as they are in torch: ReLU and max-pool as fmaxf dropped the NaN on the way.
    // The flag is loaded here and applied at the stores at the end: nothing in between waits for it.
    bool bad = bad_row && bad_row[b] != 0;
    if (sumsq) bad |= (__double2hiint(sumsq[0]) & 0x7ff00000) == 0x7ff00000;
    if (RAGGED && S < 1) {                                    // (whole block, before any barrier)
        const float qnan = __builtin_nanf("");
        for (int c = tid; c < 512; c += 256) ctx[(size_t)b * 512 + c] = qnan;
        if (logits && tid < C) logits[(size_t)b * C + tid] = qnan;
        if (logits && amax && tid == 0) amax[b] = 0;
        return;
    }
    const float* yb = y + (size_t)b * SR * 512;
    float a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = aw[lane + 64 * i];
    // four time steps per wave and round with all 32 loads issued before the first reduction (one step at a time, the
    // seven dependent load -> reduce rounds of a wave were half of this kernel's time)
    for (int t0 = 4 * wv; t0 < S; t0 += 16) {
        float v[4][8];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int i = 0; i < 8; ++i) v[k][i] = (t0 + k < S) ? yb[(size_t)(t0 + k) * 512 + lane + 64 * i] : 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float d = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) d = fmaf(v[k][i], a[i], d);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
            if (lane == 0 && t0 + k < S) sc[t0 + k] = d + ab[0];
        }
    }
    __syncthreads();
    // softmax weights once per time step (thread t), not once per (channel, time step): the exponentials were 5000
    // instructions per thread and most of this kernel's 21 us
    __shared__ float ex[ATT_MAX_S];
    float mx = -INFINITY;
    for (int t = 0; t < S; ++t) mx = fmaxf(mx, sc[t]);
    if (tid < S) ex[tid] = expf(sc[tid] - mx);
    __syncthreads();
    float den = 0.0f;
    for (int t = 0; t < S; ++t) den += ex[t];
    __syncthreads();                                          // every thread has read ex[] before it is overwritten
    if (tid < S) ex[tid] = ex[tid] / den;
    __syncthreads();
    for (int c = tid; c < 512; c += 256) {
        float acc = 0.0f;
        for (int t = 0; t < S; ++t) acc = fmaf(ex[t], yb[(size_t)t * 512 + c], acc);
        ctx[(size_t)b * 512 + c] = acc;
        cs[c] = acc;
    }
    if (!logits) return;
    __syncthreads();
    // classifier: thread = (class j = tid / 8 (+ 32), eighth of the 512 inputs); sixteen independent float4 loads per thread,
    // then a reduction over the eight lanes of a class (C <= 64)
    for (int j = tid >> 3; j < C; j += 32) {
        const int part = tid & 7;
        const float4* wr = reinterpret_cast<const float4*>(fcw + (size_t)j * 512 + part * 64);
        const float4* cr = reinterpret_cast<const float4*>(cs + part * 64);
        float d = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float4 wv4 = wr[i], c4 = cr[i];
            d = fmaf(c4.x, wv4.x, d); d = fmaf(c4.y, wv4.y, d); d = fmaf(c4.z, wv4.z, d); d = fmaf(c4.w, wv4.w, d);
        }
        d += __shfl_xor(d, 1); d += __shfl_xor(d, 2); d += __shfl_xor(d, 4);
        if (part == 0) {
            d += fcb[j];
            if (bad) d = __builtin_nanf("");
            lg[j] = d;
            logits[(size_t)b * C + j] = d;
        }
    }
    if (!amax) return;
    __syncthreads();
    if (tid == 0) {
        float best = lg[0];
        int bi = 0;
        for (int c = 1; c < C; ++c)
            if (lg[c] > best) { best = lg[c]; bi = c; }      // first maximum, as torch.argmax
        amax[b] = bi;
    }
}
static __global__ __launch_bounds__(256) void attention_pool_kernel(const float* __restrict__ y, const float* __restrict__ aw,
                                                             const float* __restrict__ ab, float* __restrict__ ctx,
                                                             int S, const float* __restrict__ fcw,
                                                             const float* __restrict__ fcb, int C,
                                                             float* __restrict__ logits, long long* __restrict__ amax,
                                                             const int* __restrict__ bad_row, const double* __restrict__ sumsq) {
    attention_pool_body<false>(y, aw, ab, ctx, S, fcw, fcb, C, logits, amax, nullptr, bad_row, sumsq);
}
static __global__ __launch_bounds__(256) void attention_pool_ragged_kernel(const float* __restrict__ y, const float* __restrict__ aw,
                                                             const float* __restrict__ ab, float* __restrict__ ctx,
                                                             int S, const float* __restrict__ fcw,
                                                             const float* __restrict__ fcb, int C,
                                                             float* __restrict__ logits, long long* __restrict__ amax,
                                                             const int* __restrict__ slen, const int* __restrict__ bad_row) {
    attention_pool_body<true>(y, aw, ab, ctx, S, fcw, fcb, C, logits, amax, slen, bad_row, nullptr);
}
#endif

