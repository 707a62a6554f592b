// Training-only device kernels of the BACKWARD: head, BatchNorm / pool / ReLU, conv1, the slab reduces of the weight gradients.
// Included by model_train_bwd.hip.  Layouts as in model_kernels.h (NHWC activations).
#pragma once
#include "model_kernels.h"
#include "train_workspace.h"

// ------------------------------------------------------------------------------------------
// The backward's loss scale for one call (train_workspace.h: sir_bwd_loss_scale), from the dlogits it was handed.  Writes pairs
// {scale, 1 / scale} of powers of two into TB_BSC: pair 0 for the call, pair 1 + b for utterance b.
//   max |dlogits| * 2^static_exp lies in [2^(x-1), 2^x); x = 8 for a mean cross-entropy far from convergence.  While x stays in
//   [BSC_X_LO, BSC_X_HI] the static scale is kept (bit for bit what a fixed scale computes); outside it the exponent moves by 8 - x,
//   which puts the scaled maximum back into [2^7, 2^8).  A zero, subnormal or non-finite maximum keeps the static scale (NaN and
//   infinity then travel through the backward as they are).
//   per_row == 0: one workgroup, pair 0 from the maximum over all of dlogits (pairs 1.. are not written).
//   per_row != 0: one wave per utterance (16 per workgroup), pair 1 + b from the maximum of row b alone -- for the data-only
//   backward under frozen statistics, where utterance b's gradients depend on row b of dlogits and nothing else; pair 0 = static.
//   demb (sir_model_train_bwd_emb; else NULL, and the pairs are bit for bit those of the maximum over dlogits alone): the gradient
//   that enters at the embedding is counted as a dlogits of |demb| * 2^BSC_EMB_Q.  head_bwd_utt adds demb to dctx = dlogits fc_w,
//   and at the reference head's initialisation (fc_w uniform within +-512^-1/2 = 2^-4.5) max |dctx| is about max |dlogits| * 2^-4.5:
//   the one large entry of a row of softmax - onehot times the largest weights of its class.  A demb of magnitude m therefore
//   loads the contractions behind the head like a dlogits of m * 2^4.5; the exponent is rounded up to 5, to the side that scales
//   down (the window [BSC_X_LO, BSC_X_HI] has two binades of room either way).  With dlogits all zero the scale follows demb alone.
//   per_row: row b's maximum is over row b of both arrays.  A non-finite demb, like a non-finite dlogits, keeps the static scale.
// ------------------------------------------------------------------------------------------
constexpr int BSC_X_LO = 6, BSC_X_HI = 10;
constexpr int BSC_EMB_Q = 5;
// |v| * 2^BSC_EMB_Q as the bits the maximum is taken over (fp32 product: infinity and NaN stay what they are, an overflow becomes
// infinity and keeps the static scale)
__device__ __forceinline__ unsigned bwd_scale_emb_bits(float v) { return __float_as_uint(v * (float)(1 << BSC_EMB_Q)) & 0x7fffffffu; }
__device__ __forceinline__ unsigned bwd_scale_emb_bits4(const float4 v) {
    return max(max(bwd_scale_emb_bits(v.x), bwd_scale_emb_bits(v.y)), max(bwd_scale_emb_bits(v.z), bwd_scale_emb_bits(v.w)));
}
__device__ __forceinline__ void bwd_scale_pair(unsigned maxbits, int static_exp, float* __restrict__ out) {
    const int e = (int)(maxbits >> 23);                       // biased exponent (the sign bit is already cleared)
    int g = static_exp;
    if (e != 0 && e != 255) {
        const int x = e - 126 + static_exp;
        if (x < BSC_X_LO || x > BSC_X_HI) g = min(max(static_exp + 8 - x, -100), 100);
    }
    out[0] = __uint_as_float((unsigned)(127 + g) << 23);
    out[1] = __uint_as_float((unsigned)(127 - g) << 23);
}
//   slen (ragged step; else NULL): a row whose clip has slen[b] < 1 steps counts as a row of zeros (its dlogits are not looked at).
static __global__ __launch_bounds__(1024) void bwd_scale_kernel(const float* __restrict__ dlogits, int B, int C, int static_exp, int per_row,
                                                                float* __restrict__ bsc, const int* __restrict__ slen, const float* __restrict__ demb) {
    __shared__ unsigned red[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (per_row) {
        const int b = blockIdx.x * 16 + wv;
        if (b < B) {
            unsigned v = lane < C && !(slen && slen[b] < 1) ? (__float_as_uint(dlogits[(size_t)b * C + lane]) & 0x7fffffffu) : 0u;
            if (demb && !(slen && slen[b] < 1)) {                 // (wave-uniform) the lane's eight elements of row b: two 16-byte loads
                const float4* r = reinterpret_cast<const float4*>(demb + (size_t)b * 512) + 2 * lane;
                v = max(v, max(bwd_scale_emb_bits4(r[0]), bwd_scale_emb_bits4(r[1])));
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
            if (lane == 0) bwd_scale_pair(v, static_exp, bsc + 2 * (1 + b));
        }
        if (blockIdx.x == 0 && tid == 0) bwd_scale_pair(0u, static_exp, bsc);
        return;
    }
    unsigned m = 0u;
    const size_t n = (size_t)B * C;
    if (slen) {
        for (size_t i = tid; i < n; i += 1024)
            if (slen[i / C] >= 1) m = max(m, __float_as_uint(dlogits[i]) & 0x7fffffffu);
    } else {
        for (size_t i = tid; i < n; i += 1024) m = max(m, __float_as_uint(dlogits[i]) & 0x7fffffffu);
    }
    if (demb) {                                                   // 128 float4 per row; a clip without steps (ragged) is not looked at
        const size_t n4 = (size_t)B * 128;
        for (size_t i = tid; i < n4; i += 1024)
            if (!(slen && slen[i >> 7] < 1)) m = max(m, bwd_scale_emb_bits4(reinterpret_cast<const float4*>(demb)[i]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if (lane == 0) red[wv] = m;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < 16; ++i) m = max(m, red[i]);
        bwd_scale_pair(m, static_exp, bsc);
    }
}

// ------------------------------------------------------------------------------------------
// head backward: fc + attention pooling (models.py:63-67)
//   dctx = dlogits fc_w (+ demb, the gradient that enters at the embedding: sir_model_train_bwd_emb)
//   w = softmax_t(y a + b);  dw_t = <dctx, y_t>;  ds_t = w_t (dw_t - sum w dw)
//   dy_t = w_t dctx + ds_t a;  per-utterance partials of d attention.weight / d attention.bias
// one workgroup per utterance
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void head_bwd_utt(int b, const float* __restrict__ dlogits, const float* __restrict__ fcw,
                                             const float* __restrict__ y, const float* __restrict__ aw,
                                             const float* __restrict__ ab, float* __restrict__ dy,
                                             float* __restrict__ daw_part, float* __restrict__ dab_part,
                                             int S, int C, float gscale, int Sl, const float* __restrict__ demb) {
    // Sl <= S: the utterance's own steps (ragged step; S otherwise) -- scores, softmax and sums over t < Sl, dy rows t >= Sl are zeros
    __shared__ float dctx[512];
    __shared__ float sc[ATT_MAX_S], ds[ATT_MAX_S];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* yb = y + (size_t)b * S * 512;
    if (Sl < 1) {                                             // (whole block, before any barrier: a clip of width 0 -- nothing but zeros)
        for (int c = tid; c < 512; c += 256) {
            for (int t = 0; t < S; ++t) dy[((size_t)b * S + t) * 512 + c] = 0.0f;
            daw_part[(size_t)b * 512 + c] = 0.0f;
        }
        if (tid == 0) dab_part[b] = 0.0f;
        return;
    }
    for (int c = tid; c < 512; c += 256) {
        float a = 0.0f;
        for (int j = 0; j < C; ++j) a = fmaf(dlogits[(size_t)b * C + j], fcw[(size_t)j * 512 + c], a);
        if (demb) a += demb[(size_t)b * 512 + c];                 // (workgroup-uniform; NULL: the statements of before, the same bits)
        dctx[c] = a;
    }
    float a8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a8[i] = aw[lane + 64 * i];
    __syncthreads();
    float dc8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) dc8[i] = dctx[lane + 64 * i];
    // four time steps per wave and round, all 32 loads issued before the first reduction (cf. attention_pool_kernel)
    for (int t0 = 4 * wv; t0 < Sl; t0 += 16) {
        float v[4][8];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int i = 0; i < 8; ++i) v[k][i] = (t0 + k < Sl) ? yb[(size_t)(t0 + k) * 512 + lane + 64 * i] : 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float d = 0.0f, g = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                d = fmaf(v[k][i], a8[i], d);
                g = fmaf(v[k][i], dc8[i], g);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { d += __shfl_xor(d, o); g += __shfl_xor(g, o); }
            if (lane == 0 && t0 + k < Sl) { sc[t0 + k] = d + ab[0]; ds[t0 + k] = g; }   // ds holds dw_t for now
        }
    }
    __syncthreads();
    // softmax weights once per time step (thread t)
    __shared__ float ex[ATT_MAX_S];
    float mx = -INFINITY;
    for (int t = 0; t < Sl; ++t) mx = fmaxf(mx, sc[t]);
    for (int t = tid; t < Sl; t += 256) ex[t] = expf(sc[t] - mx);
    __syncthreads();
    float den = 0.0f;
    for (int t = 0; t < Sl; ++t) den += ex[t];
    float wdw = 0.0f;
    for (int t = 0; t < Sl; ++t) wdw = fmaf(ex[t] / den, ds[t], wdw);
    __syncthreads();
    for (int t = tid; t < Sl; t += 256) {
        const float w = ex[t] / den;
        const float dst = w * (ds[t] - wdw);
        sc[t] = w;                 // now the attention weight
        ds[t] = dst;               // now d score
    }
    __syncthreads();
    float dsum = 0.0f;
    for (int t = 0; t < Sl; ++t) dsum += ds[t];
    for (int c = tid; c < 512; c += 256) {
        const float dc = dctx[c], ac = aw[c];
        float da = 0.0f;
        for (int t = 0; t < Sl; ++t) {
            dy[((size_t)b * S + t) * 512 + c] = gscale * fmaf(sc[t], dc, ds[t] * ac);     // (the backward's loss scale: a power of two, exact)
            da = fmaf(ds[t], yb[(size_t)t * 512 + c], da);
        }
        for (int t = Sl; t < S; ++t) dy[((size_t)b * S + t) * 512 + c] = 0.0f;
        daw_part[(size_t)b * 512 + c] = da;
    }
    if (tid == 0) dab_part[b] = dsum;
}

// out[n] = sum_r in[r][n]   (deterministic column sums: bias / attention gradients)
static __global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ in, int rows, int ld, int n_cols,
                                                      float* __restrict__ out) {
    __shared__ float red[4][64];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
    float a = 0.0f;
    if (col < n_cols) {
#pragma unroll 8
        for (int r = part; r < rows; r += 4) a += in[(size_t)r * ld + col];
    }
    red[part][threadIdx.x & 63] = a;
    __syncthreads();
    if (part == 0 && col < n_cols) out[col] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// attention.weight (512 column sums of daw_part [rows][512]) and attention.bias (the sum of dab_part [rows]) in ONE launch:
// blocks 0..7 take 64 columns each, block 8 the bias
static __global__ __launch_bounds__(256) void head_colsum_kernel(const float* __restrict__ daw_part, const float* __restrict__ dab_part,
                                                                  int rows, float* __restrict__ out_w, float* __restrict__ out_b) {
    __shared__ float red[4][64];
    const bool bias = blockIdx.x == 8;
    const int l = threadIdx.x & 63, col = blockIdx.x * 64 + l, part = threadIdx.x >> 6;
    float a = 0.0f;
    if (!bias) {
#pragma unroll 8
        for (int r = part; r < rows; r += 4) a += daw_part[(size_t)r * 512 + col];     // 8 loads in flight, added in row order
    }
    else { for (int r = threadIdx.x; r < rows; r += 256) a += dab_part[r]; }
    if (bias) {                                   // 256 partial sums -> one value, fixed order
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    }
    red[part][l] = a;
    __syncthreads();
    if (part == 0 && (!bias || l == 0)) {
        const float v = red[0][l] + red[1][l] + red[2][l] + red[3][l];
        if (bias) { if (out_b) out_b[0] = v; } else if (out_w) out_w[col] = v;     // (NULL = that gradient is not wanted)
    }
}

// the four GRU bias gradients of one layer in ONE launch: column sums of bsum_i / bsum_h [rows][1536] (blockIdx.y selects
// the array), columns [0, 768) -> direction 0, [768, 1536) -> direction 1
static __global__ __launch_bounds__(256) void gru_bias_colsum_kernel(const float* __restrict__ bsum_i, const float* __restrict__ bsum_h, int rows,
                                                                      float* __restrict__ bi0, float* __restrict__ bi1,
                                                                      float* __restrict__ bh0, float* __restrict__ bh1, const float* __restrict__ bsc) {
    const float unscale = bsc[1];
    __shared__ float red[4][64];
    const float* in = blockIdx.y ? bsum_h : bsum_i;
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;     // col < 1536 (grid.x = 24)
    float a = 0.0f;
#pragma unroll 8
    for (int r = part; r < rows; r += 4) a += in[(size_t)r * 1536 + col];
    red[part][threadIdx.x & 63] = a;
    __syncthreads();
    if (part == 0) {
        const float v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        float* out = blockIdx.y ? (col < 768 ? bh0 : bh1) : (col < 768 ? bi0 : bi1);
        if (out) out[col < 768 ? col : col - 768] = v * unscale;     // (NULL = that gradient is not wanted)
    }
}

// first stage for tall inputs: out[chunk][n] = sum over the rows of chunk `blockIdx.y` (then colsum_kernel)
static __global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ in, int rows, int ld, int n_cols,
                                                                     float* __restrict__ out) {
    __shared__ float red[4][64];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
    const int per = (rows + gridDim.y - 1) / gridDim.y;
    const int r0 = blockIdx.y * per, r1 = min(rows, r0 + per);
    float a = 0.0f;
    if (col < n_cols) {
#pragma unroll 8
        for (int r = r0 + part; r < r1; r += 4) a += in[(size_t)r * ld + col];
    }
    red[part][threadIdx.x & 63] = a;
    __syncthreads();
    if (part == 0 && col < n_cols)
        out[(size_t)blockIdx.y * n_cols + col] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// dfc_w[j][c] = sum_b dlogits[b][j] ctx[b][c];  dfc_b[j] = sum_b dlogits[b][j]
//   grid (C, 2): block (j, half) owns 256 columns c; the dlogits column is staged in LDS once and the loop over
//   the batch is unrolled so that the ctx loads pipeline (the first version ran one dependent load per iteration)
__device__ __forceinline__ void fc_wgrad_block(int j, int half, const float* __restrict__ dlogits, const float* __restrict__ ctx,
                                               float* __restrict__ dw, float* __restrict__ db, int B, int C, const int* __restrict__ slen) {
    // slen (ragged step; else NULL): a row of a clip without steps counts as dlogits = 0, and its ctx row (NaN) is not used as data
    __shared__ float dl[1024];
    const int c = half * 256 + threadIdx.x;
    float a = 0.0f, sb = 0.0f;
    for (int b0 = 0; b0 < B; b0 += 1024) {
        const int nb = min(1024, B - b0);
        __syncthreads();
        for (int i = threadIdx.x; i < nb; i += 256) dl[i] = (slen && slen[b0 + i] < 1) ? 0.0f : dlogits[(size_t)(b0 + i) * C + j];
        __syncthreads();
        int b = 0;
        if (slen) {                                    // (a product with dl == 0 adds nothing: selected away, so that 0 x NaN cannot appear)
            for (; b < nb; ++b) { a = fmaf(dl[b], dl[b] != 0.0f ? ctx[(size_t)(b0 + b) * 512 + c] : 0.0f, a); sb += dl[b]; }
        }
        for (; b + 8 <= nb; b += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = ctx[(size_t)(b0 + b + u) * 512 + c];
#pragma unroll
            for (int u = 0; u < 8; ++u) { a = fmaf(dl[b + u], v[u], a); sb += dl[b + u]; }
        }
        for (; b < nb; ++b) { a = fmaf(dl[b], ctx[(size_t)(b0 + b) * 512 + c], a); sb += dl[b]; }
    }
    if (dw) dw[(size_t)j * 512 + c] = a;          // (NULL = that gradient is not wanted)
    if (db && c == 0) db[j] = sb;
}

// head backward, ONE launch for two independent jobs (both only need dlogits): workgroups [0, B) = one utterance each
// (head_bwd_utt: fc + attention pooling backward, per-utterance attention partials; its dy output -- and with it everything the
// rest of the backward computes -- carries the loss scale of bwd_scale_kernel, pair 0 or the row's own); workgroups [B, B + 2 C) = the fc weight /
// bias gradients (fc_wgrad_block).  head_colsum_kernel adds the attention partials afterwards.
static __global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ fcw,
                                                              const float* __restrict__ y, const float* __restrict__ aw,
                                                              const float* __restrict__ ab, const float* __restrict__ ctx,
                                                              float* __restrict__ dy, float* __restrict__ daw_part,
                                                              float* __restrict__ dab_part, float* __restrict__ d_fc_w,
                                                              float* __restrict__ d_fc_b, int B, int S, int C, const float* __restrict__ bsc, int row_scaled,
                                                              const int* __restrict__ slen, const float* __restrict__ demb) {
    // slen (ragged step, sir_model_train_bwd_ragged; else NULL): utterance b has slen[b] <= S steps of its own
    if ((int)blockIdx.x >= B) {
        const int i = blockIdx.x - B;
        fc_wgrad_block(i >> 1, i & 1, dlogits, ctx, d_fc_w, d_fc_b, B, C, slen);
        return;
    }
    head_bwd_utt(blockIdx.x, dlogits, fcw, y, aw, ab, dy, daw_part, dab_part, S, C, bsc[row_scaled ? 2 * (1 + blockIdx.x) : 0],
                 slen ? max(0, min(S, slen[blockIdx.x])) : S, demb);
}

// Reads two buffers and keeps nothing: a software prefetch into the last-level cache, launched on the backward's side stream (model_train_bwd.hip:
// layer 0's saved gates and outputs ahead of its BPTT)
static __global__ __launch_bounds__(256) void cache_touch_kernel(const float4* __restrict__ a, size_t na, const float4* __restrict__ b, size_t nb,
                                                                  float* __restrict__ sink) {
    float acc = 0.0f;
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < na; i += stride) { const float4 v = a[i]; acc += v.x + v.y + v.z + v.w; }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += stride) { const float4 v = b[i]; acc += v.x + v.y + v.z + v.w; }
    if (acc == 123456.789f) sink[0] = acc;               // (never true in practice; keeps the loads)
}

// out_j[i] = sum_z slabs_j[z][i] for up to four jobs (blockIdx.y) with a common slab count; slab stride = n_j
struct SlabJobs { const float* src[4]; float* out[4]; size_t n[4]; };
static __global__ void slab_reduce_jobs_kernel(SlabJobs jobs, int nslab, const float* __restrict__ bsc) {
    const float unscale = bsc[1];
    const int j = blockIdx.y;
    const size_t n = jobs.n[j];
    const float* __restrict__ s = jobs.src[j];
    float* __restrict__ o = jobs.out[j];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float a = 0.0f;
#pragma unroll 8
        for (int z = 0; z < nslab; ++z) a += s[(size_t)z * n + i];
        o[i] = a * unscale;
    }
}

// ------------------------------------------------------------------------------------------
// backward through max-pool -> ReLU -> BatchNorm (batch statistics).
//   da: gradient wrt the pooled output (NHWC [B][Hp][Wp][C], or the GRU layout when GRU_IN)
//   z : raw conv output [B][H][W][C];  y = z*scale+shift
//   dy(pixel) = da if the pixel is the first maximum of its 2x2 window and y > 0, else 0
// pass 1 (bn_bwd_reduce): per-block partial sums of dy and dy*xhat per channel (-> dbeta, dgamma)
// pass 2 (bn_bwd_dz): dz = gamma*invstd*(dy - mean(dy) - xhat*mean(dy*xhat)) at full resolution
// ------------------------------------------------------------------------------------------
template <bool GRU_IN>
__device__ __forceinline__ float4 load_da4(const float* __restrict__ da, int b, int py, int px, int c4, int Hp, int Wp,
                                           int C) {
    if (!GRU_IN) return *reinterpret_cast<const float4*>(da + (((size_t)b * Hp + py) * Wp + px) * C + c4 * 4);
    const float* o = da + ((size_t)b * Wp + px) * ((size_t)C * Hp) + (size_t)(c4 * 4) * Hp + py;
    return make_float4(o[0], o[Hp], o[2 * Hp], o[3 * Hp]);
}

// gradient reaching pixel (dy,dx) of the window, per channel component
__device__ __forceinline__ float route1(float y00, float y01, float y10, float y11, int pos, float g) {
    float best = y00; int arg = 0;
    if (y01 > best) { best = y01; arg = 1; }
    if (y10 > best) { best = y10; arg = 2; }
    if (y11 > best) { best = y11; arg = 3; }
    return (arg == pos && best > 0.0f) ? g : 0.0f;
}

// The same two sums from the POOLED activations a = pool(relu(bn(z))): dy = da wherever a > 0 (the window's maximum passed
// the ReLU; a zero gradient otherwise), and at that maximum y = a, hence xhat = (y - beta) / gamma = (a - beta) / gamma.
// Reads a and da (2 x 52 MB for conv2) instead of z and da (210 + 52 MB).  A channel whose gamma is too small for the
// division (|gamma| < 1e-2 (1 + |beta|): rounding of a would be amplified) takes the z path for its windows.
__device__ __forceinline__ bool bn_gamma_ok(float gamma, float beta) { return fabsf(gamma) >= 1e-2f * (1.0f + fabsf(beta)); }

// NHWC activations [B][Hp][Wp][C]; same block / thread mapping and partial layout as bn_bwd_reduce_kernel<false>
static __global__ __launch_bounds__(256) void bn_bwd_reduce_pooled_kernel(
    const float* __restrict__ a, const float* __restrict__ da, const float* __restrict__ z, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
    const float* __restrict__ invstd, float2* __restrict__ part, int B, int H, int W, int C, int Hp, int Wp, int pix_per_block,
    const int* __restrict__ wlim) {
    // wlim (ragged step; else NULL): the pooled gradient of clip b counts as zero at columns >= wlim[b] (the data gradient of the conv
    // above spills one column past the clip's width)
    __shared__ float rs[256], rq[256];
    const int c4n = C / 4;
    const int lanes_c = c4n < 64 ? c4n : 64;
    const int pl = 256 / lanes_c;
    const int c4 = threadIdx.x % lanes_c, pslot = threadIdx.x / lanes_c;
    const size_t npix = (size_t)B * Hp * Wp;
    const size_t p0 = (size_t)blockIdx.x * pix_per_block;
    for (int cc = c4; cc < c4n; cc += lanes_c) {
        const float4 gm = *reinterpret_cast<const float4*>(gamma + cc * 4), bt = *reinterpret_cast<const float4*>(beta + cc * 4);
        const bool fast = bn_gamma_ok(gm.x, bt.x) && bn_gamma_ok(gm.y, bt.y) && bn_gamma_ok(gm.z, bt.z) && bn_gamma_ok(gm.w, bt.w);
        float4 sdy = make_float4(0.f, 0.f, 0.f, 0.f), sdx = sdy;
        if (fast) {
            const float4 rg = make_float4(1.0f / gm.x, 1.0f / gm.y, 1.0f / gm.z, 1.0f / gm.w);
            for (int i = pslot; i < pix_per_block; i += pl) {
                const size_t p = p0 + i;
                if (p >= npix) break;
                if (wlim && (int)(p % Wp) >= wlim[p / ((size_t)Wp * Hp)]) continue;
                const float4 av = *reinterpret_cast<const float4*>(a + p * C + cc * 4);
                const float4 g = *reinterpret_cast<const float4*>(da + p * C + cc * 4);
                const float dx_ = av.x > 0.0f ? g.x : 0.0f, dy_ = av.y > 0.0f ? g.y : 0.0f;
                const float dz_ = av.z > 0.0f ? g.z : 0.0f, dw_ = av.w > 0.0f ? g.w : 0.0f;
                sdy.x += dx_; sdy.y += dy_; sdy.z += dz_; sdy.w += dw_;
                sdx.x = fmaf(dx_, (av.x - bt.x) * rg.x, sdx.x); sdx.y = fmaf(dy_, (av.y - bt.y) * rg.y, sdx.y);
                sdx.z = fmaf(dz_, (av.z - bt.z) * rg.z, sdx.z); sdx.w = fmaf(dw_, (av.w - bt.w) * rg.w, sdx.w);
            }
        } else {
            const float4 s = *reinterpret_cast<const float4*>(scale + cc * 4), t = *reinterpret_cast<const float4*>(shift + cc * 4);
            const float4 mu = *reinterpret_cast<const float4*>(mean + cc * 4), is = *reinterpret_cast<const float4*>(invstd + cc * 4);
            for (int i = pslot; i < pix_per_block; i += pl) {
                const size_t p = p0 + i;
                if (p >= npix) break;
                const int px = p % Wp, py = (p / Wp) % Hp, b = p / ((size_t)Wp * Hp);
                if (wlim && px >= wlim[b]) continue;
                const float4 g = *reinterpret_cast<const float4*>(da + p * C + cc * 4);
                float4 zz[4], yy[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    zz[q] = *reinterpret_cast<const float4*>(z + (((size_t)b * H + 2 * py + (q >> 1)) * W + 2 * px + (q & 1)) * C + cc * 4);
                    yy[q] = make_float4(fmaf(zz[q].x, s.x, t.x), fmaf(zz[q].y, s.y, t.y), fmaf(zz[q].z, s.z, t.z), fmaf(zz[q].w, s.w, t.w));
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float dx_ = route1(yy[0].x, yy[1].x, yy[2].x, yy[3].x, q, g.x);
                    const float dy_ = route1(yy[0].y, yy[1].y, yy[2].y, yy[3].y, q, g.y);
                    const float dz_ = route1(yy[0].z, yy[1].z, yy[2].z, yy[3].z, q, g.z);
                    const float dw_ = route1(yy[0].w, yy[1].w, yy[2].w, yy[3].w, q, g.w);
                    sdy.x += dx_; sdy.y += dy_; sdy.z += dz_; sdy.w += dw_;
                    sdx.x = fmaf(dx_, (zz[q].x - mu.x) * is.x, sdx.x); sdx.y = fmaf(dy_, (zz[q].y - mu.y) * is.y, sdx.y);
                    sdx.z = fmaf(dz_, (zz[q].z - mu.z) * is.z, sdx.z); sdx.w = fmaf(dw_, (zz[q].w - mu.w) * is.w, sdx.w);
                }
            }
        }
        const float vs[4] = {sdy.x, sdy.y, sdy.z, sdy.w}, vq[4] = {sdx.x, sdx.y, sdx.z, sdx.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            __syncthreads();
            rs[threadIdx.x] = vs[e]; rq[threadIdx.x] = vq[e];
            __syncthreads();
            if (pslot == 0) {
                float acc = 0.0f, q2 = 0.0f;
                for (int k = 0; k < pl; ++k) { acc += rs[k * lanes_c + c4]; q2 += rq[k * lanes_c + c4]; }
                part[(size_t)blockIdx.x * C + cc * 4 + e] = make_float2(acc, q2);
            }
        }
    }
}

// GRU-layout activations [B * Wp][C * Hp] with feature = c * Hp + py and C * Hp = 1024, Hp = 8: thread = one float4 of a
// row (four py of ONE channel), block = rows_per_block rows; lanes 2c, 2c + 1 hold the two halves of channel c.
static __global__ __launch_bounds__(256) void bn_bwd_reduce_pooled_gru_kernel(
    const float* __restrict__ a, const float* __restrict__ da, const float* __restrict__ z, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
    const float* __restrict__ invstd, float2* __restrict__ part, int rows, int H, int W, int Wp, int rows_per_block) {
    constexpr int C = 128, Hp = 8;
    const int tid = threadIdx.x, c = tid >> 1, py0 = (tid & 1) * 4;
    const float gm = gamma[c], bt = beta[c];
    const int r0 = blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
    float sdy = 0.0f, sdx = 0.0f;
    if (bn_gamma_ok(gm, bt)) {
        const float rg = 1.0f / gm;
        for (int r = r0; r < r1; ++r) {
            const float4 av = *reinterpret_cast<const float4*>(a + (size_t)r * 1024 + tid * 4);
            const float4 g = *reinterpret_cast<const float4*>(da + (size_t)r * 1024 + tid * 4);
            const float d0 = av.x > 0.0f ? g.x : 0.0f, d1 = av.y > 0.0f ? g.y : 0.0f;
            const float d2 = av.z > 0.0f ? g.z : 0.0f, d3 = av.w > 0.0f ? g.w : 0.0f;
            sdy += (d0 + d1) + (d2 + d3);
            sdx = fmaf(d0, (av.x - bt) * rg, sdx); sdx = fmaf(d1, (av.y - bt) * rg, sdx);
            sdx = fmaf(d2, (av.z - bt) * rg, sdx); sdx = fmaf(d3, (av.w - bt) * rg, sdx);
        }
    } else {
        const float s = scale[c], t = shift[c], mu = mean[c], is = invstd[c];
        for (int r = r0; r < r1; ++r) {
            const int b = r / Wp, px = r - b * Wp;
            const float4 g4 = *reinterpret_cast<const float4*>(da + (size_t)r * 1024 + tid * 4);
            const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int py = py0 + e;
                float zz[4], yy[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    zz[q] = z[(((size_t)b * H + 2 * py + (q >> 1)) * W + 2 * px + (q & 1)) * C + c];
                    yy[q] = fmaf(zz[q], s, t);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float d_ = route1(yy[0], yy[1], yy[2], yy[3], q, gv[e]);
                    sdy += d_;
                    sdx = fmaf(d_, (zz[q] - mu) * is, sdx);
                }
            }
        }
    }
    static_assert(C * Hp == 1024, "one 1024-float row per 256 threads");
    sdy += __shfl_xor(sdy, 1);
    sdx += __shfl_xor(sdx, 1);
    if ((tid & 1) == 0) part[(size_t)blockIdx.x * C + c] = make_float2(sdy, sdx);
}

// sums the (sum dy, sum dy*xhat) partials -> dbeta, dgamma and the two per-channel means used by dz
static __global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float2* __restrict__ part, int nblk, int C, double count,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                               float* __restrict__ mdy, float* __restrict__ mdyx, const float* __restrict__ bsc) {
    const float unscale = bsc[1];
    __shared__ double rs[256], rq[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    double s = 0.0, q = 0.0;
#pragma unroll 4
    for (int i = tid; i < nblk; i += 256) { const float2 v = part[(size_t)i * C + c]; s += v.x; q += v.y; }
    rs[tid] = s; rq[tid] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { rs[tid] += rs[tid + o]; rq[tid] += rq[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        if (dbeta) dbeta[c] = (float)rs[0] * unscale;   // parameter gradients leave the loss scale; the means below feed dz and keep it
        if (dgamma) dgamma[c] = (float)rq[0] * unscale; // (NULL = that gradient is not wanted)
        mdy[c] = (float)(rs[0] / count);
        mdyx[c] = (float)(rq[0] / count);
    }
}

// frozen statistics: the same ordered sum of the partials, but only dbeta / dgamma come out of it (dz has no mean terms, so
// nothing downstream waits for this kernel); either output may be NULL
static __global__ __launch_bounds__(256) void bn_bwd_finalize_frozen_kernel(const float2* __restrict__ part, int nblk, int C,
                                                                      float* __restrict__ dgamma, float* __restrict__ dbeta, const float* __restrict__ bsc) {
    const float unscale = bsc[1];
    __shared__ double rs[256], rq[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    double s = 0.0, q = 0.0;
#pragma unroll 4
    for (int i = tid; i < nblk; i += 256) { const float2 v = part[(size_t)i * C + c]; s += v.x; q += v.y; }
    rs[tid] = s; rq[tid] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { rs[tid] += rs[tid + o]; rq[tid] += rq[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        if (dbeta) dbeta[c] = (float)rs[0] * unscale;
        if (dgamma) dgamma[c] = (float)rq[0] * unscale;
    }
}

// first maximum of the 2x2 window (PyTorch's max-pool tie rule: row-major scan, strict >), -1 if ReLU blocks it
__device__ __forceinline__ int route_arg(float y00, float y01, float y10, float y11) {
    float best = y00; int arg = 0;
    if (y01 > best) { best = y01; arg = 1; }
    if (y10 > best) { best = y10; arg = 2; }
    if (y11 > best) { best = y11; arg = 3; }
    return best > 0.0f ? arg : -1;
}

// thread = one 2x2 window x 4 channels: the four z values are read once (a thread per PIXEL re-read its three window
// neighbours for the routing: 5 loads per output against 1.25 here), the pooled gradient once per window
// FROZEN (running statistics): dz = gamma * invstd_running * dy -- the mean terms are gone, and with them the mean / invstd /
// mdy / mdyx reads (pass NULL) and the dependence on the reduce pass; z is still read for the routing
// RAGGED (ragged step): the pooled gradient of clip b counts as zero at columns >= wlim[b] -- `da` is not read there
template <bool GRU_IN, bool FROZEN = false, bool RAGGED = false>
__global__ __launch_bounds__(256) void bn_bwd_dz_kernel(const float* __restrict__ z, const float* __restrict__ da,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         const float* __restrict__ mean, const float* __restrict__ invstd,
                                                         const float* __restrict__ mdy, const float* __restrict__ mdyx,
                                                         float* __restrict__ dz, int B, int H, int W, int C, int Hp, int Wp,
                                                         const int* __restrict__ wlim = nullptr) {
    const int c4n = C / 4, Hc = (H + 1) / 2, Wc = (W + 1) / 2;           // cells cover an odd last row / column too
    const size_t total = (size_t)B * Hc * Wc * c4n;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        int cc, cx, cy, b;
        if (GRU_IN) {
            // the pooled gradient is [b][px][c][py] here: with the cell ROW as the fastest thread index eight lanes read one 32-byte
            // row of it (channel-fastest threads picked one float out of every row: 373 MB of traffic for 236 MB of work)
            cy = idx % Hc;
            size_t rest = idx / Hc;
            cc = rest % c4n; rest /= c4n;
            cx = rest % Wc;
            b = rest / Wc;
        } else {
            cc = idx % c4n;
            size_t rest = idx / c4n;
            cx = rest % Wc; rest /= Wc;
            cy = rest % Hc;
            b = rest / Hc;
        }
        const float4 s = *reinterpret_cast<const float4*>(scale + cc * 4), t = *reinterpret_cast<const float4*>(shift + cc * 4);
        float4 mu = make_float4(0.f, 0.f, 0.f, 0.f), is = mu, m1 = mu, m2 = mu;
        if (!FROZEN) {
            mu = *reinterpret_cast<const float4*>(mean + cc * 4); is = *reinterpret_cast<const float4*>(invstd + cc * 4);
            m1 = *reinterpret_cast<const float4*>(mdy + cc * 4); m2 = *reinterpret_cast<const float4*>(mdyx + cc * 4);
        }
        float4 zq[4];
        bool ok[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int y = 2 * cy + (q >> 1), x = 2 * cx + (q & 1);
            ok[q] = y < H && x < W;
            zq[q] = ok[q] ? *reinterpret_cast<const float4*>(z + (((size_t)b * H + y) * W + x) * C + cc * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        int ax = -1, ay = -1, az = -1, aw = -1;
        if (cy < Hp && cx < Wp && (!RAGGED || cx < wlim[b])) {           // pooled window (all four pixels exist)
            g = load_da4<GRU_IN>(da, b, cy, cx, cc, Hp, Wp, C);
            ax = route_arg(fmaf(zq[0].x, s.x, t.x), fmaf(zq[1].x, s.x, t.x), fmaf(zq[2].x, s.x, t.x), fmaf(zq[3].x, s.x, t.x));
            ay = route_arg(fmaf(zq[0].y, s.y, t.y), fmaf(zq[1].y, s.y, t.y), fmaf(zq[2].y, s.y, t.y), fmaf(zq[3].y, s.y, t.y));
            az = route_arg(fmaf(zq[0].z, s.z, t.z), fmaf(zq[1].z, s.z, t.z), fmaf(zq[2].z, s.z, t.z), fmaf(zq[3].z, s.z, t.z));
            aw = route_arg(fmaf(zq[0].w, s.w, t.w), fmaf(zq[1].w, s.w, t.w), fmaf(zq[2].w, s.w, t.w), fmaf(zq[3].w, s.w, t.w));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!ok[q]) continue;
            const int y = 2 * cy + (q >> 1), x = 2 * cx + (q & 1);
            float4 o;
            if (FROZEN) {
                o.x = s.x * (ax == q ? g.x : 0.0f); o.y = s.y * (ay == q ? g.y : 0.0f);
                o.z = s.z * (az == q ? g.z : 0.0f); o.w = s.w * (aw == q ? g.w : 0.0f);
                *reinterpret_cast<float4*>(dz + (((size_t)b * H + y) * W + x) * C + cc * 4) = o;
                continue;
            }
            o.x = s.x * ((ax == q ? g.x : 0.0f) - m1.x - (zq[q].x - mu.x) * is.x * m2.x);
            o.y = s.y * ((ay == q ? g.y : 0.0f) - m1.y - (zq[q].y - mu.y) * is.y * m2.y);
            o.z = s.z * ((az == q ? g.z : 0.0f) - m1.z - (zq[q].z - mu.z) * is.z * m2.z);
            o.w = s.w * ((aw == q ? g.w : 0.0f) - m1.w - (zq[q].w - mu.w) * is.w * m2.w);
            *reinterpret_cast<float4*>(dz + (((size_t)b * H + y) * W + x) * C + cc * 4) = o;
        }
    }
}

// ------------------------------------------------------------------------------------------
// conv1 block backward (conv1 output is recomputed from the features, never stored).
//   pass 1: partial (sum dy, sum dy*xhat) per channel      -> bn_bwd_finalize_kernel
//   pass 2: dz = gamma*invstd*(dy - mean dy - xhat*mean(dy xhat)), dW1[c][tap] partials per block
// Same tiling as conv1_bn_relu_pool_kernel: block = 4 x 32 pooled pixels, lane&31 = channel.
// ------------------------------------------------------------------------------------------
// MODE 0: pass 1;  MODE 1: pass 2 (needs mdy / mdyx);  MODE 2: both in ONE pass -- (sum dy, sum dy*xhat, A[9]) with
// A[tap] = sum dy * x_tap, the only data-dependent part of the weight gradient: the mean terms of dz are closed forms in the
// input moments of conv1_moments_kernel (conv1_bwd_finalize_kernel).
// RAGGED (ragged step): frame columns >= xlim[b] of clip b are the image edge -- read as zeros, whatever bits they hold, as in the
// forward -- and the pooled gradient counts as zero at columns >= wlim[b] (conv2's data gradient spills one column past the width).
template <int MODE, bool RAGGED = false>
__global__ __launch_bounds__(256) void conv1_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ da, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, const float* __restrict__ mean,
                                                         const float* __restrict__ invstd, const float* __restrict__ mdy,
                                                         const float* __restrict__ mdyx, float* __restrict__ part,
                                                         int H, int W, int Hp, int Wp, const int* __restrict__ wlim = nullptr,
                                                         const int* __restrict__ xlim = nullptr) {
    constexpr bool WGRAD = MODE == 1;
    constexpr int NV = MODE == 0 ? 2 : (MODE == 1 ? 9 : 11);
    __shared__ float tile[C1_TR * C1_TC];
    __shared__ float red[8 * 32 * NV];
    const int b = blockIdx.z, py0 = blockIdx.y * C1_PROWS, px0 = blockIdx.x * C1_PCOLS;
    const int tid = threadIdx.x, c = tid & 31, slot = tid >> 5;
    const float* xb = x + (size_t)b * H * W;
    int Wx = W, Wl = Wp;                                      // columns of the image that hold data / of the pooled gradient that count
    if constexpr (RAGGED) { Wx = max(0, min(W, xlim[b])); Wl = max(0, min(Wp, wlim[b])); }
    for (int i = tid; i < C1_TR * C1_TC; i += 256) {
        const int ty = i / C1_TC, tx = i - ty * C1_TC;
        const int gy = 2 * py0 - 1 + ty, gx = 2 * px0 - 1 + tx;
        tile[i] = (gy >= 0 && gy < H && gx >= 0 && gx < Wx) ? xb[(size_t)gy * W + gx] : 0.0f;
    }
    float wk[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) wk[i] = w[c * 9 + i];
    const float s = scale[c], t = shift[c], mu = mean[c], is = invstd[c];
    const float m1 = WGRAD ? mdy[c] : 0.0f, m2 = WGRAD ? mdyx[c] : 0.0f;
    float accv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) accv[i] = 0.0f;
    __syncthreads();
    for (int i = 0; i < (C1_PROWS * C1_PCOLS) / 8; ++i) {
        const int pp = slot + 8 * i, pyl = pp / C1_PCOLS, pxl = pp % C1_PCOLS;
        const int py = py0 + pyl, px = px0 + pxl;
        if (2 * py >= H || 2 * px >= W) continue;
        float in[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k) in[r][k] = tile[(2 * pyl + r) * C1_TC + 2 * pxl + k];
        float a[4], yv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v = 0.0f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) v = fmaf(in[(q >> 1) + ky][(q & 1) + kx], wk[ky * 3 + kx], v);
            a[q] = v;
            yv[q] = fmaf(v, s, t);
        }
        const bool pooled = (py < Hp && px < Wl);
        const float g = pooled ? da[(((size_t)b * Hp + py) * Wp + px) * 32 + c] : 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gy = 2 * py + (q >> 1), gx = 2 * px + (q & 1);
            if (gy >= H || gx >= W) continue;
            const float dyq = pooled ? route1(yv[0], yv[1], yv[2], yv[3], q, g) : 0.0f;
            const float xh = (a[q] - mu) * is;
            if (MODE != 1) {
                accv[0] += dyq;
                accv[1] = fmaf(dyq, xh, accv[1]);
                if (MODE == 2) {
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            accv[2 + ky * 3 + kx] = fmaf(dyq, in[(q >> 1) + ky][(q & 1) + kx], accv[2 + ky * 3 + kx]);
                            // keeps the SLP vectoriser from pairing these into v_pk_fma_f32: the shifted windows are not
                            // register-pair aligned, and the pairing cost 160 v_mov per pixel (166 us instead of ~100)
                            asm volatile("" : "+v"(accv[2 + ky * 3 + kx]));
                        }
                }
            } else {
                const float dzq = s * (dyq - m1 - xh * m2);
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx)
                        accv[ky * 3 + kx] = fmaf(dzq, in[(q >> 1) + ky][(q & 1) + kx], accv[ky * 3 + kx]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) red[(slot * 32 + c) * NV + i] = accv[i];
    __syncthreads();
    const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    for (int o = tid; o < 32 * NV; o += 256) {
        float v = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) v += red[k * 32 * NV + o];
        part[blk * 32 * NV + o] = v;           // !WGRAD: float2 (sum dy, sum dy xhat) per channel
    }
}

// totals[c][11] = (sum dy, sum dy*xhat, A[9]) summed over the blocks;  M = input moments (forward).  Thread (c, tap):
//   dW[c][tap] = s_c (A[tap] - m1 S[tap] - m2 invstd_c (sum_t w_c[t] R[t][tap] - mean_c S[tap])),   m1 = sum dy / N, m2 = sum dy*xhat / N
// (dz = s (dy - m1 - xhat m2), xhat = (z - mean) invstd, z = sum_t w[t] x_t), evaluated in double; thread (c, 0) also writes
// dbeta = sum dy and dgamma = sum dy*xhat.
// m1_out / m2_out (both or neither; NULL = not wanted): the two means as floats, still carrying the loss scale, for
// conv1_bwd_data_kernel.
static __global__ void conv1_bwd_finalize_kernel(const float* __restrict__ totals, const double* __restrict__ M, const float* __restrict__ w,
                                                 const float* __restrict__ scale, const float* __restrict__ mean,
                                                 const float* __restrict__ invstd, double count, float* __restrict__ dgamma,
                                                 float* __restrict__ dbeta, float* __restrict__ dw, const float* __restrict__ bsc,
                                                 float* __restrict__ m1_out, float* __restrict__ m2_out) {
    const float unscale = bsc[1];
    const int idx = threadIdx.x;
    if (idx >= 288) return;
    const int c = idx / 9, tap = idx % 9;
    const double sdy = totals[c * 11], sdx = totals[c * 11 + 1], A = totals[c * 11 + 2 + tap];
    const double m1 = sdy / count, m2 = sdx / count;
    double zx = 0.0;                                             // sum z * x_tap
    for (int t = 0; t < 9; ++t) zx += (double)w[c * 9 + t] * M[t <= tap ? c1_r_index(t, tap) : c1_r_index(tap, t)];
    const double xhx = (double)invstd[c] * (zx - (double)mean[c] * M[tap]);
    if (dw) dw[c * 9 + tap] = (float)((double)scale[c] * (A - m1 * M[tap] - m2 * xhx)) * unscale;     // (NULL = not wanted)
    if (tap == 0) {
        if (dbeta) dbeta[c] = (float)sdy * unscale;
        if (dgamma) dgamma[c] = (float)sdx * unscale;
        if (m1_out) { m1_out[c] = (float)m1; m2_out[c] = (float)m2; }
    }
}

// frozen statistics: dz = s dy, so dW[c][tap] = s_c A[tap], dbeta = sum dy, dgamma = sum dy*xhat are plain sums of the same
// totals (xhat from the running statistics); no input moments.  Any output may be NULL.
static __global__ void conv1_bwd_finalize_frozen_kernel(const float* __restrict__ totals, const float* __restrict__ scale,
                                                        float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dw,
                                                        const float* __restrict__ bsc) {
    const float unscale = bsc[1];
    const int idx = threadIdx.x;
    if (idx >= 288) return;
    const int c = idx / 9, tap = idx % 9;
    if (dw) dw[c * 9 + tap] = (float)((double)scale[c] * (double)totals[c * 11 + 2 + tap]) * unscale;
    if (tap == 0) {
        if (dbeta) dbeta[c] = totals[c * 11] * unscale;
        if (dgamma) dgamma[c] = totals[c * 11 + 1] * unscale;
    }
}

// ------------------------------------------------------------------------------------------
// conv1 block DATA gradient: d(loss)/d(features), the last link of the chain (sir_model_train_bwd_x).
//   dx[b][h][w] = unscale * sum_c sum_{kh,kw} w1[c][kh][kw] * dz1[b][c][h + 1 - kh][w + 1 - kw]        (dz1 = 0 outside the image)
// dz1 is never stored in global memory.  A workgroup owns C1D_TH x C1D_TW input pixels of one utterance.  It stages the features of
// its tile with a 3-pixel halo in LDS, then, for one half of the channels at a time:
//   recompute -- thread = one 2x2 pooling window x 4 channels, windows aligned to even coordinates and covering the tile with a
//     one-window halo: z1 as the forward's chain of nine fmas in tap order ky * 3 + kx, y = fma(z, scale, shift), the routing of
//     conv1_bwd_kernel (route1: first maximum, strict >, blocked by the ReLU); one 16-byte read of da1 (channel-innermost NHWC)
//     per thread and window;  dz = s (dy - m1 - xhat m2), or s dy with FROZEN statistics;  a pixel outside the image gets 0, a
//     pixel of a column the pooling drops gets dy = 0;  dz goes to LDS as [pixel][16 channels + 4 pad] (the tile + 1 pixel around);
//   gather -- thread = two vertically adjacent output pixels: 16 channels x 9 taps from 4 x 3 16-byte LDS reads per four channels
//     (pixel stride 80 bytes: the 16 lanes of a ds_read_b128 group fall on 16 different 16-byte slots), weights from scalar loads.
// Everything is summed in a fixed order: the result is bit-reproducible.  Output written, not accumulated, without the loss scale.
// ------------------------------------------------------------------------------------------
constexpr int C1D_TH = 16, C1D_TW = 32;                       // output tile (even: pooling windows stay whole)
constexpr int C1D_XR = C1D_TH + 6, C1D_XC = C1D_TW + 6;       // feature tile with its 3-pixel halo
constexpr int C1D_CR = C1D_TH / 2 + 2, C1D_CC = C1D_TW / 2 + 2;   // pooling windows with a one-window halo
constexpr int C1D_ZR = C1D_TH + 2, C1D_ZC = C1D_TW + 2;       // dz pixels kept: the tile + 1 pixel around
constexpr int C1D_ZS = 20;                                    // floats per dz pixel in LDS: 16 channels + 4 pad
static_assert(C1D_TH * C1D_TW == 2 * 256, "two output pixels per thread");

// RAGGED (ragged step; FROZEN only): frame columns >= xlim[b] are the image edge (read as zeros, as in the forward), the pooled
// gradient counts as zero at columns >= wlim[b], and dx is written as zero at columns >= xlim[b] (the transposed convolution spills
// one column past an even width; the last column of an odd width is inside the clip: conv1 read it, and it keeps its gradient).
template <bool FROZEN, bool RAGGED = false>
__global__ __launch_bounds__(256, 3) void conv1_bwd_data_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ da, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, const float* __restrict__ mdy,
                                                              const float* __restrict__ mdyx, float* __restrict__ dx,
                                                              int H, int W, int Hp, int Wp, const float* __restrict__ bsc, int row_scaled,
                                                              const int* __restrict__ wlim = nullptr, const int* __restrict__ xlim = nullptr) {
    const float unscale = bsc[row_scaled ? 2 * (1 + blockIdx.z) + 1 : 1];    // (the utterance's own scale: bwd_scale_kernel)
    __shared__ float xt[C1D_XR * C1D_XC];
    __shared__ __attribute__((aligned(16))) float dzs[C1D_ZR * C1D_ZC * C1D_ZS];
    const int b = blockIdx.z, h0 = blockIdx.y * C1D_TH, w0 = blockIdx.x * C1D_TW;
    const int tid = threadIdx.x;
    const float* xb = x + (size_t)b * H * W;
    int Wx = W, Wl = Wp;
    if constexpr (RAGGED) { Wx = max(0, min(W, xlim[b])); Wl = max(0, min(Wp, wlim[b])); }
    for (int i = tid; i < C1D_XR * C1D_XC; i += 256) {
        const int ty = i / C1D_XC, tx = i - ty * C1D_XC;
        const int gy = h0 - 3 + ty, gx = w0 - 3 + tx;
        xt[i] = (gy >= 0 && gy < H && gx >= 0 && gx < Wx) ? xb[(size_t)gy * W + gx] : 0.0f;
    }
    const int lc = tid & 31, rp = tid >> 5;                   // gather: output column, pair of output rows
    float acc0 = 0.0f, acc1 = 0.0f;
    constexpr int NIT = (C1D_CR * C1D_CC * 4 + 255) / 256;    // recompute items (window, 4 channels) per thread and channel half
    for (int half = 0; half < 2; ++half) {
        // ---- recompute: dz of 16 channels into LDS ----
        const int c0 = half * 16 + (tid & 3) * 4;             // this thread's four channels (256 % 4 == 0: the same for all its items)
        float4 g[NIT];
        int wcy[NIT], wcx[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {                    // all da1 reads of the half are issued first
            const int cell = (it * 256 + tid) >> 2;
            wcy[it] = cell / C1D_CC; wcx[it] = cell - wcy[it] * C1D_CC;
            const int gcy = (h0 >> 1) - 1 + wcy[it], gcx = (w0 >> 1) - 1 + wcx[it];
            const bool pooled = cell < C1D_CR * C1D_CC && gcy >= 0 && gcy < Hp && gcx >= 0 && gcx < Wl;
            g[it] = pooled ? *reinterpret_cast<const float4*>(da + (((size_t)b * Hp + gcy) * Wp + gcx) * 32 + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (!pooled) wcy[it] |= 0x100;                    // (bit 8: no pooled gradient for this window)
            if (cell >= C1D_CR * C1D_CC) wcy[it] = -1;
        }
        float wk[4][9], s[4], t[4], mu[4], is[4], m1[4], m2[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int i = 0; i < 9; ++i) wk[e][i] = w[(c0 + e) * 9 + i];
            s[e] = scale[c0 + e]; t[e] = shift[c0 + e];
            mu[e] = FROZEN ? 0.0f : mean[c0 + e]; is[e] = FROZEN ? 0.0f : invstd[c0 + e];
            m1[e] = FROZEN ? 0.0f : mdy[c0 + e]; m2[e] = FROZEN ? 0.0f : mdyx[c0 + e];
        }
        __syncthreads();                                      // xt is staged (first half) / the last half's gather is done
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (wcy[it] < 0) continue;
            const bool pooled = !(wcy[it] & 0x100);
            const int cy = wcy[it] & 0xff, cx = wcx[it];
            float in[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k) in[r][k] = xt[(2 * cy + r) * C1D_XC + 2 * cx + k];
            const float gv[4] = {g[it].x, g[it].y, g[it].z, g[it].w};
            float o[4][4];                                    // [window pixel][channel]
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a[4], yv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v = 0.0f;
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) v = fmaf(in[(q >> 1) + ky][(q & 1) + kx], wk[e][ky * 3 + kx], v);
                    a[q] = v;
                    yv[q] = fmaf(v, s[e], t[e]);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float dyq = pooled ? route1(yv[0], yv[1], yv[2], yv[3], q, gv[e]) : 0.0f;
                    if (FROZEN) o[q][e] = s[e] * dyq;
                    else { const float xh = (a[q] - mu[e]) * is[e]; o[q][e] = s[e] * (dyq - m1[e] - xh * m2[e]); }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int zr = 2 * cy - 1 + (q >> 1), zc = 2 * cx - 1 + (q & 1);      // pixel (h0 - 1 + zr, w0 - 1 + zc)
                if (zr < 0 || zr >= C1D_ZR || zc < 0 || zc >= C1D_ZC) continue;
                const int gy = h0 - 1 + zr, gx = w0 - 1 + zc;
                const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
                *reinterpret_cast<float4*>(&dzs[(zr * C1D_ZC + zc) * C1D_ZS + (tid & 3) * 4]) =
                    inside ? make_float4(o[q][0], o[q][1], o[q][2], o[q][3]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        __syncthreads();
        // ---- gather: rows 2 rp, 2 rp + 1 of the tile, column lc; dz rows 2 rp .. 2 rp + 3, columns lc .. lc + 2 ----
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
            float4 v[4][3];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) v[r][k] = *reinterpret_cast<const float4*>(&dzs[((2 * rp + r) * C1D_ZC + lc + k) * C1D_ZS + c4 * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float* wc = w + (half * 16 + c4 * 4 + e) * 9;      // (uniform address: scalar loads)
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const float wv = wc[kh * 3 + kw];
                        const float4 u0 = v[2 - kh][2 - kw], u1 = v[3 - kh][2 - kw];
                        acc0 = fmaf(wv, e == 0 ? u0.x : (e == 1 ? u0.y : (e == 2 ? u0.z : u0.w)), acc0);
                        acc1 = fmaf(wv, e == 0 ? u1.x : (e == 1 ? u1.y : (e == 2 ? u1.z : u1.w)), acc1);
                    }
            }
        }
    }
    const int gx = w0 + lc, gy = h0 + 2 * rp;
    if (gx < W) {
        const bool in = !RAGGED || gx < Wx;
        if (gy < H) dx[((size_t)b * H + gy) * W + gx] = in ? acc0 * unscale : 0.0f;
        if (gy + 1 < H) dx[((size_t)b * H + gy + 1) * W + gx] = in ? acc1 * unscale : 0.0f;
    }
}

// dW[co][ci][tap] = sum_blk slab[blk][tap][co][ci], in two ordered (deterministic) passes: WGR_PARTS partial sums over
// interleaved-free contiguous slab ranges (grid.y), then their sum + the transpose to the torch layout
static __global__ __launch_bounds__(256) void wgrad_reduce_partial_kernel(const float* __restrict__ slab, int nblk, int total4,
                                                                     float* __restrict__ part) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;       // float4 index into one slab
    if (idx >= total4) return;
    const int per = (nblk + WGR_PARTS - 1) / WGR_PARTS, k0 = blockIdx.y * per, k1 = min(nblk, k0 + per);
    const float4* s4 = reinterpret_cast<const float4*>(slab);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int k = k0;
    for (; k + 4 <= k1; k += 4) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = s4[(size_t)(k + u) * total4 + idx];
#pragma unroll
        for (int u = 0; u < 4; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
    }
    for (; k < k1; ++k) {
        const float4 v = s4[(size_t)k * total4 + idx];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    reinterpret_cast<float4*>(part)[(size_t)blockIdx.y * total4 + idx] = acc;
}
static __global__ void wgrad_reduce_kernel(const float* __restrict__ part, int nparts, int cin, int cout, float* __restrict__ dw, const float* __restrict__ bsc) {
    const float unscale = bsc[1];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;       // (tap, co, ci), ci fastest
    const int total = 9 * cout * cin;
    if (idx >= total) return;
    const int ci = idx % cin, co = (idx / cin) % cout, tap = idx / (cin * cout);
    float s = 0.0f;
#pragma unroll 8
    for (int k = 0; k < nparts; ++k) s += part[(size_t)k * total + idx];
    dw[((size_t)co * cin + ci) * 9 + tap] = s * unscale;
}
