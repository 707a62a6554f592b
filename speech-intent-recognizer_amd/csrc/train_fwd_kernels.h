// Training-only device kernels of the FORWARD: BatchNorm with batch statistics (conv1's from input moments), the inter-layer
// dropout, and the one-launch weight preparation of the whole step.  Included by model_train_fwd.hip.  Layouts as in
// model_kernels.h (NHWC activations).
#pragma once
#include "model_kernels.h"
#include "bf16x6_kernels.h"
#include "conv_wino2_f16x3_kernel.h"
#include "gru_frag_prep.h"
#include "train_workspace.h"

// ------------------------------------------------------------------------------------------
// BatchNorm with batch statistics
// ------------------------------------------------------------------------------------------

// ------------------------------------------------------------------------------------------
// conv1 BatchNorm statistics WITHOUT computing conv1: z_c = sum_t w_c[t] x_t with x_t the nine shifted copies of the
// (zero-padded) feature image, hence
//     sum z_c   = sum_t w_c[t] S[t]                       S[t]     = sum_pixels x_t
//     sum z_c^2 = sum_{t,u} w_c[t] w_c[u] R[t][u]         R[t][u]  = sum_pixels x_t x_u
// -- 9 + 45 moments of the INPUT, the same for all 32 channels (one pass over 13 MB instead of recomputing 105 M conv
// outputs x 32 channels).  The backward reuses them for the mean terms of the weight gradient (conv1_bwd_finalize_kernel).
// Moment layout M[54]: S[0..8], then R packed by rows, t <= u: index 9 + t*9 - t*(t-1)/2 + (u - t).
// ------------------------------------------------------------------------------------------

// wave WV of a block accumulates the moments [14 WV, 14 WV + 14) -- over ALL pixels of a tile -- so that each of the 54 sums
// is reduced across 64 lanes exactly once per block (with 54 accumulators in every thread the wave reductions cost more than
// the accumulation itself)
constexpr int C1_MPW = 14;
template <int WV>
__device__ __forceinline__ void c1_moments_accum(const float (&v)[9], float (&m)[C1_MPW]) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        if (t / C1_MPW == WV) m[t - C1_MPW * WV] += v[t];
#pragma unroll
        for (int u = t; u < 9; ++u)
            if (c1_r_index(t, u) / C1_MPW == WV) m[c1_r_index(t, u) - C1_MPW * WV] = fmaf(v[t], v[u], m[c1_r_index(t, u) - C1_MPW * WV]);
    }
}

// block (g, b) walks the 8 x 64-pixel tiles g, g + gridDim.x, ... of image b; part[54][gridDim.y * gridDim.x] (moment-major: the
// reduce kernel then reads contiguous rows -- block-major rows of 54 floats made it a 216-byte-stride gather, 37 us for 442 KB)
static __global__ __launch_bounds__(256) void conv1_moments_kernel(const float* __restrict__ x, float* __restrict__ part, int H, int W,
                                                                    int tiles_x, int tiles_y) {
    __shared__ float tile[C1_TR * C1_TC];
    const int b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* xb = x + (size_t)b * H * W;
    float m[C1_MPW];
#pragma unroll
    for (int i = 0; i < C1_MPW; ++i) m[i] = 0.0f;
    for (int tl = blockIdx.x; tl < tiles_x * tiles_y; tl += gridDim.x) {
        const int y0 = 2 * (tl / tiles_x) * C1_PROWS, x0 = 2 * (tl % tiles_x) * C1_PCOLS;
        __syncthreads();                                   // previous tile consumed
        for (int i = tid; i < C1_TR * C1_TC; i += 256) {
            const int ty = i / C1_TC, tx = i - ty * C1_TC;
            const int gy = y0 - 1 + ty, gx = x0 - 1 + tx;
            tile[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? xb[(size_t)gy * W + gx] : 0.0f;
        }
        __syncthreads();
        for (int k = 0; k < (4 * C1_PROWS * C1_PCOLS) / 64; ++k) {          // 512 pixels / 64 lanes
            const int pix = lane + 64 * k, ly = pix / (2 * C1_PCOLS), lx = pix % (2 * C1_PCOLS);
            if (y0 + ly >= H || x0 + lx >= W) continue;
            float v[9];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) v[ky * 3 + kx] = tile[(ly + ky) * C1_TC + lx + kx];
            switch (wv) {                                   // wave-uniform
                case 0: c1_moments_accum<0>(v, m); break;
                case 1: c1_moments_accum<1>(v, m); break;
                case 2: c1_moments_accum<2>(v, m); break;
                default: c1_moments_accum<3>(v, m); break;
            }
        }
    }
    const size_t blk = (size_t)b * gridDim.x + blockIdx.x, nblk = (size_t)gridDim.x * gridDim.y;
#pragma unroll
    for (int i = 0; i < C1_MPW; ++i) {
        float a = m[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0 && C1_MPW * wv + i < C1_NMOM) part[(size_t)(C1_MPW * wv + i) * nblk + blk] = a;
    }
}

// M[i] = sum over blocks (double); one block per moment
static __global__ __launch_bounds__(256) void conv1_moments_reduce_kernel(const float* __restrict__ part, int nblk, double* __restrict__ M) {
    __shared__ double rs[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
#pragma unroll 8
    for (int r = tid; r < nblk; r += 256) s += part[(size_t)i * nblk + r];
    rs[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) rs[tid] += rs[tid + o];
        __syncthreads();
    }
    if (tid == 0) M[i] = rs[0];
}

__device__ __forceinline__ void bn_finalize_channel(double sum, double sumsq, double count, int c, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float* __restrict__ run_mean,
                                                    float* __restrict__ run_var, float momentum, float* __restrict__ scale,
                                                    float* __restrict__ shift, float* __restrict__ save_mean,
                                                    float* __restrict__ save_invstd, unsigned int* __restrict__ status) {
    // (the PARAMETERS only: batch statistics that are not finite come from the features, which the head kernel answers for)
    sir_flag_bn_param(sir_finite(gamma[c]) && sir_finite(beta[c]), status);
    const double mean = sum / count;
    double var = sumsq / count - mean * mean;
    if (var < 0.0) var = 0.0;
    const float invstd = (float)(1.0 / sqrt(var + (double)SIR_BN_EPS));
    const float sc = gamma[c] * invstd;
    scale[c] = sc;
    shift[c] = beta[c] - (float)mean * sc;
    save_mean[c] = (float)mean;
    save_invstd[c] = invstd;
    const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
    run_mean[c] = (1.0f - momentum) * run_mean[c] + momentum * (float)mean;
    run_var[c] = (1.0f - momentum) * run_var[c] + momentum * (float)unbiased;
}

// per channel: (sum z, sum z^2) from the moments and the nine weights, then the usual BatchNorm finalisation; 32 threads
static __global__ void conv1_bn_from_moments_kernel(const double* __restrict__ M, const float* __restrict__ w, double count,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float* __restrict__ run_mean, float* __restrict__ run_var, float momentum,
                                                    float* __restrict__ scale, float* __restrict__ shift,
                                                    float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                    unsigned int* __restrict__ status) {
    const int c = threadIdx.x;
    if (c >= 32) return;
    double wk[9];
    bool ok = true;
    for (int t = 0; t < 9; ++t) { wk[t] = (double)w[c * 9 + t]; ok = ok && sir_finite(w[c * 9 + t]); }
    sir_flag_bn_param(ok, status);
    double sum = 0.0, sumsq = 0.0;
    for (int t = 0; t < 9; ++t) {
        sum += wk[t] * M[t];
        sumsq += wk[t] * wk[t] * M[c1_r_index(t, t)];
        for (int u = t + 1; u < 9; ++u) sumsq += 2.0 * wk[t] * wk[u] * M[c1_r_index(t, u)];
    }
    bn_finalize_channel(sum, sumsq, count, c, gamma, beta, run_mean, run_var, momentum, scale, shift, save_mean, save_invstd, status);
}

// partial (sum, sumsq) [nblk][C] -> batch mean / biased var -> folded scale/shift for the forward,
// saved mean / invstd for the backward, running statistics updated in place
// (momentum 0.1, unbiased variance: torch.nn.BatchNorm2d training semantics).  One block per channel.
static __global__ __launch_bounds__(256) void bn_finalize_kernel(const float2* __restrict__ stats, int nblk, int C, double count,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ run_mean, float* __restrict__ run_var,
                                                           float momentum, float* __restrict__ scale,
                                                           float* __restrict__ shift, float* __restrict__ save_mean,
                                                           float* __restrict__ save_invstd, unsigned int* __restrict__ status) {
    __shared__ double rs[256], rq[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    double s = 0.0, q = 0.0;
#pragma unroll 4
    for (int i = tid; i < nblk; i += 256) {
        const float2 v = stats[(size_t)i * C + c];
        s += v.x;
        q += v.y;
    }
    rs[tid] = s; rq[tid] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { rs[tid] += rs[tid + o]; rq[tid] += rq[tid + o]; }
        __syncthreads();
    }
    if (tid == 0)
        bn_finalize_channel(rs[0], rq[0], count, c, gamma, beta, run_mean, run_var, momentum, scale, shift, save_mean, save_invstd, status);
}

// Frozen statistics (bnK.eval() inside a training step): the running mean / variance take the place of the batch ones in the
// four per-channel arrays that the apply kernels and the backward read; nothing is reduced and the running statistics stay as
// they are.  One thread per channel.
static __global__ void bn_fold_running_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                              const float* __restrict__ run_mean, const float* __restrict__ run_var, int C,
                                              float* __restrict__ scale, float* __restrict__ shift,
                                              float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                              const float* __restrict__ w1, int n1, unsigned int* __restrict__ status) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float mean = run_mean[c];
    const float invstd = (float)(1.0 / sqrt((double)run_var[c] + (double)SIR_BN_EPS));
    const float sc = gamma[c] * invstd;
    scale[c] = sc;
    shift[c] = beta[c] - mean * sc;
    save_mean[c] = mean;
    save_invstd[c] = invstd;
    bool ok = sir_finite(sc) && sir_finite(beta[c] - mean * sc);      // (w1 / n1: conv1's weights beside bn1's, as prep_bn_kernel)
    for (int j = c; j < n1; j += C) ok = ok && sir_finite(w1[j]);
    sir_flag_bn_param(ok, status);
}

// z (raw conv output, NHWC [B][H][W][C]) -> relu(bn(z)) -> 2x2 max-pool.
// GRU_OUT = false: NHWC [B][Hp][Wp][C];  true: [B][Wp][C*Hp] with feature = c*Hp + py (models.py:55-57)
// An output that is not below `limit` -- the range inside which the backward's single-accumulator f16x3 contractions take this
// tensor exactly (a2: wgrad_wino_f16x3_kernel.h, 256; x0: gemm_tn2_f16x3_kernel.h, 512) -- raises bit 12 of the status word.
// RAGGED (sir_model_train_fwd_ragged): clip b's pooled map is wlim[b] <= Wp columns wide; the columns behind it are written as
// zeros and their z is not read -- the next stage runs at full width and reads them as the clip's right edge.
template <bool GRU_OUT, bool RAGGED = false>
__global__ __launch_bounds__(256) void bn_relu_pool_kernel(const float* __restrict__ z, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float* __restrict__ out,
                                                            int B, int H, int W, int C, int Hp, int Wp, float limit,
                                                            unsigned int* __restrict__ status, const int* __restrict__ wlim = nullptr) {
    const int c4n = C / 4;
    bool beyond = false;
    const size_t total = (size_t)B * Hp * Wp * c4n;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        int c4, px, py, b;
        if (!GRU_OUT) {
            c4 = idx % c4n;
            size_t rest = idx / c4n;
            px = rest % Wp; rest /= Wp;
            py = rest % Hp;
            b = rest / Hp;
        } else {                                      // py fastest: the lanes of a wave then fill whole 32-byte sectors of
            py = idx % Hp;                            // the [c*Hp + py] feature rows (c4 fastest scattered single floats)
            size_t rest = idx / Hp;
            c4 = rest % c4n; rest /= c4n;
            px = rest % Wp;
            b = rest / Wp;
        }
        const float4 s = *reinterpret_cast<const float4*>(scale + c4 * 4);
        const float4 t = *reinterpret_cast<const float4*>(shift + c4 * 4);
        float4 best = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool live = !RAGGED || px < min(Wp, wlim[b]);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                if (!live) continue;
                const float4 v = *reinterpret_cast<const float4*>(
                    z + (((size_t)b * H + 2 * py + dy) * W + 2 * px + dx) * C + c4 * 4);
                best.x = fmaxf(best.x, fmaf(v.x, s.x, t.x));
                best.y = fmaxf(best.y, fmaf(v.y, s.y, t.y));
                best.z = fmaxf(best.z, fmaf(v.z, s.z, t.z));
                best.w = fmaxf(best.w, fmaf(v.w, s.w, t.w));
            }
        beyond |= !(fmaxf(fmaxf(best.x, best.y), fmaxf(best.z, best.w)) < limit);
        if (!GRU_OUT) {
            *reinterpret_cast<float4*>(out + (((size_t)b * Hp + py) * Wp + px) * C + c4 * 4) = best;
        } else {
            float* o = out + ((size_t)b * Wp + px) * ((size_t)C * Hp) + (size_t)(c4 * 4) * Hp + py;
            o[0] = best.x; o[Hp] = best.y; o[2 * Hp] = best.z; o[3 * Hp] = best.w;
        }
    }
    if (beyond) __hip_atomic_fetch_or(status, SIR_STATUS_ACT_RANGE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------
// inter-layer GRU dropout (models.py:32, p = 0.5 in train()): counter-based keep mask, a pure
// function of (seed, element index) so the backward pass regenerates it.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool dropout_keep(unsigned long long seed, size_t idx, float p) {
    unsigned long long x = seed ^ (idx * 0x9E3779B97F4A7C15ull);
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return (float)(unsigned)(x >> 40) * (1.0f / 16777216.0f) >= p;
}

// out = dropout(in) AND the f16x2 planes [2][n] of out (the A operand of the next layer's input projection) in one pass;
// one thread = 8 consecutive elements (n is a multiple of 8: rows of 512)
static __global__ __launch_bounds__(256) void dropout_split2h_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                      unsigned short* __restrict__ planes, size_t n, float p,
                                                                      unsigned long long seed) {
    const float sc = 1.0f / (1.0f - p);
    for (size_t i8 = (size_t)blockIdx.x * 256 + threadIdx.x; i8 < n / 8; i8 += (size_t)gridDim.x * 256) {
        const size_t i = i8 * 8;
        float v[8];
        *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(in + i);
        *reinterpret_cast<float4*>(v + 4) = *reinterpret_cast<const float4*>(in + i + 4);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = dropout_keep(seed, i + e, p) ? v[e] * sc : 0.0f;
        const float4 v0 = make_float4(v[0], v[1], v[2], v[3]), v1 = make_float4(v[4], v[5], v[6], v[7]);
        *reinterpret_cast<float4*>(out + i) = v0;
        *reinterpret_cast<float4*>(out + i + 4) = v1;
        uint2 h0, l0, h1, l1;
        split2h_quad(v0, h0, l0);
        split2h_quad(v1, h1, l1);
        *reinterpret_cast<uint4*>(planes + i) = make_uint4(h0.x, h0.y, h1.x, h1.y);
        *reinterpret_cast<uint4*>(planes + n + i) = make_uint4(l0.x, l0.y, l1.x, l1.y);
    }
}

// Ragged step: zero where the clip has nothing, so that what runs at full width behind reads zeros, not what an earlier call left.
//   rows form (cols == 0): a [B][S][row_floats] buffer, rows t >= lim[b] of clip b (the GRU outputs: the ragged recurrence stores no
//     row behind a clip's last step, and the next projection, both weight-gradient GEMMs and h(t + 1) of the reverse direction's
//     last step read them);  grid (S, B)
//   columns form: an NHWC map [B][H][W][C], columns x >= lim[b] (conv1's map: the ragged conv1 kernel stores lim[b] columns);  grid (H, B)
static __global__ __launch_bounds__(256) void ragged_zero_tail_kernel(float* __restrict__ a, const int* __restrict__ lim, int H, int W, int C,
                                                                       int cols) {
    const int b = blockIdx.y, l = max(0, lim[b]);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!cols) {                                               // H = S rows of W floats
        const int t = blockIdx.x;
        if (t < l) return;
        float4* row = reinterpret_cast<float4*>(a + ((size_t)b * H + t) * W);
        for (int i = threadIdx.x; i < W / 4; i += 256) row[i] = z4;
        return;
    }
    if (l >= W) return;
    float4* row = reinterpret_cast<float4*>(a + (((size_t)b * H + blockIdx.x) * W + l) * C);
    for (int i = threadIdx.x; i < (W - l) * C / 4; i += 256) row[i] = z4;
}

// W_hh regrouped by 4 gate rows, [192][256][4] (PREP_WHH_BWD)
__device__ __forceinline__ void prep_whh_bwd_elem(const float* __restrict__ w, float* __restrict__ wr4, int idx) {
    if (idx >= 768 * 256) return;                                 // over 768*256, layout [row/4][k][4]
    const int e = idx & 3, k = (idx >> 2) & 255, r4 = idx >> 10;
    wr4[idx] = w[(size_t)(r4 * 4 + e) * 256 + k];
}

// Every per-step re-layout of the weights (they change with each optimizer step) in ONE launch: a dozen ~5 us launches
// otherwise.  Job j owns blocks [block0[j], block0[j+1]).
enum PrepKind {
    PREP_SPLIT2H = 0,               // split2h_rows (a = ld_in = K, b = rows)
    PREP_CONV_W_BF16X3 = 1,         // prep_conv_w_bf16x3 (a = cin, b = cout): nine taps, direct fallback
    PREP_CONV_WT_BF16X3 = 2,        // prep_conv_wT_bf16x3 (a = cin_f, b = cout_f)
    PREP_WHH_BWD = 3,               // prep_whh_bwd
    PREP_CONV_W_WINO_BF16X3 = 4,    // prep_conv_w_wino_bf16x3 (a = cin, b = cout): first-generation Winograd fallback
    PREP_CONV_WT_WINO_BF16X3 = 5,   // prep_conv_wT_wino_bf16x3 (a = cin_f, b = cout_f)
    PREP_CONV_W_WINO_F16X3 = 6,     // the f16x3 forms of 4 / 5 (conv_wino2_f16x3_kernel.h)
    PREP_CONV_WT_WINO_F16X3 = 7,
    PREP_WHH_QUAD = 8,              // W_hh as the resident fragments of the forward / backward cluster recurrence (gru_frag_prep.h)
    PREP_WHH_BWD_QUAD = 9
};
constexpr int PREP_MAX_JOBS = 20;
struct PrepJobs {
    const float* src[PREP_MAX_JOBS];
    void* dst[PREP_MAX_JOBS];
    int kind[PREP_MAX_JOBS], a[PREP_MAX_JOBS], b[PREP_MAX_JOBS];
    int block0[PREP_MAX_JOBS + 1];
    int njobs;
    unsigned int* status;        // the handle's status word (kinds 6 / 7 flag conv weights outside the f16x3 range, 0 / 8 GRU weights)
};
static __global__ __launch_bounds__(256) void train_prep_kernel(PrepJobs jobs) {
    int j = 0;
    while (j + 1 < jobs.njobs && (int)blockIdx.x >= jobs.block0[j + 1]) ++j;
    const int lb = blockIdx.x - jobs.block0[j], nb = jobs.block0[j + 1] - jobs.block0[j];
    const int idx = lb * 256 + threadIdx.x;
    const float* __restrict__ src = jobs.src[j];
    switch (jobs.kind[j]) {
        case PREP_SPLIT2H: split2h_rows(src, jobs.a[j], (unsigned short*)jobs.dst[j], (size_t)jobs.b[j], jobs.a[j], (size_t)idx, (size_t)nb * 256, jobs.status); break;
        case PREP_CONV_W_BF16X3: prep_conv_w_bf16x3_elem(src, (unsigned short*)jobs.dst[j], jobs.a[j], jobs.b[j], idx); break;
        case PREP_CONV_WT_BF16X3: prep_conv_wT_bf16x3_elem(src, (unsigned short*)jobs.dst[j], jobs.a[j], jobs.b[j], idx); break;
        case PREP_CONV_W_WINO_BF16X3: prep_conv_w_wino_bf16x3_elem(src, (unsigned short*)jobs.dst[j], jobs.a[j], jobs.b[j], idx); break;
        case PREP_CONV_WT_WINO_BF16X3: prep_conv_wT_wino_bf16x3_elem(src, (unsigned short*)jobs.dst[j], jobs.a[j], jobs.b[j], idx); break;
        case PREP_CONV_W_WINO_F16X3: prep_conv_w_wino_f16x3_elem(src, (unsigned short*)jobs.dst[j], jobs.a[j], jobs.b[j], idx, jobs.status); break;
        case PREP_CONV_WT_WINO_F16X3: prep_conv_wT_wino_f16x3_elem(src, (unsigned short*)jobs.dst[j], jobs.a[j], jobs.b[j], idx, jobs.status); break;
        case PREP_WHH_QUAD: prep_whh_quad_elem(src, (uint4*)jobs.dst[j], idx, jobs.status); break;
        case PREP_WHH_BWD_QUAD: prep_whh_bwd_quad_elem(src, (uint4*)jobs.dst[j], idx); break;
        default: prep_whh_bwd_elem(src, (float*)jobs.dst[j], idx); break;
    }
}
