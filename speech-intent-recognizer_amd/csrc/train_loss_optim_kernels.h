// Training-only device kernels of the loss and the optimizer: cross-entropy, multi-tensor Adam and its variants, the global
// gradient norm.  Included by train_loss_optim.hip.
#pragma once
#include "sir_internal.h"
#include "ce_loss_rows.h"

// ------------------------------------------------------------------------------------------
// cross-entropy (mean) forward + gradient wrt logits (ce_loss_rows.h), a single head: the segment is the whole row.
// single workgroup, deterministic reduction.  SOFT: sir_ce_loss_soft's targets; SOFT = false is sir_ce_loss's kernel.
// ------------------------------------------------------------------------------------------
template <int CMAX, bool SOFT>
static __global__ __launch_bounds__(256) void ce_loss_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                       int B, int C, float* __restrict__ loss, float* __restrict__ dlogits,
                                                       float grad_scale, unsigned int* status,
                                                       const long long* __restrict__ labels_b, const float* __restrict__ lam,
                                                       float eps) {
    __shared__ float red[256];
    __shared__ int cnt[256];
    const float nvalid = ce_valid_rows(labels, B, 1, 0, cnt);
    const float acc = ce_rows<CMAX, SOFT>(logits, labels, labels_b, lam, eps, B, C, 0, 1, 0, C, nvalid, grad_scale, dlogits, status);
    const float sum = ce_block_sum(acc, red);
    if (threadIdx.x == 0) loss[0] = sum / nvalid;
}

// ------------------------------------------------------------------------------------------
// multi-tensor Adam, coupled L2 weight decay (torch.optim.Adam, train.py:246-250): one launch
// updates every parameter tensor.  Tensors are described by value in the kernel argument.
// ------------------------------------------------------------------------------------------
#define SIR_ADAM_MAX_TENSORS 32
#define SIR_ADAM_CHUNK 4096

struct AdamTensors {
    float* p[SIR_ADAM_MAX_TENSORS];
    const float* g[SIR_ADAM_MAX_TENSORS];
    float* m[SIR_ADAM_MAX_TENSORS];
    float* v[SIR_ADAM_MAX_TENSORS];
    long long n[SIR_ADAM_MAX_TENSORS];
    int first_block[SIR_ADAM_MAX_TENSORS + 1];
    int count;
};

// the EMA shadow of each tensor (sir_adam_step_ex): a kernel argument of its own, so that the launches of sir_adam_step /
// sir_adam_step_clipped keep the arguments they have
struct AdamShadow {
    float* e[SIR_ADAM_MAX_TENSORS];
};

// One block's 4096-element chunk.  CLIP: the gradient is g * coef (rounded to fp32 first, exactly what an in-place
// clip_grad_norm_ would have left in memory) before the weight-decay term.
// DECOUPLED (torch.optim.AdamW): p is first multiplied by decay_f = 1 - lr * weight_decay (formed on the host, rounded to
// fp32 once; the product is rounded too, as torch's p.mul_ leaves it), then the update runs on the gradient alone:
// `weight_decay` is not read.  EMA: shadow = fma(d, shadow, (1 - d) * p_new) with the p_new this thread has just formed --
// one more load and store in the same pass, two roundings.  Both false: the code of the two switches is not there.
template <bool CLIP, bool DECOUPLED = false, bool EMA = false>
__device__ __forceinline__ void adam_chunk(const AdamTensors& ts, float lr, float beta1, float beta2, float eps, float weight_decay,
                                           float bc1, float bc2_sqrt, float coef, float decay_f = 1.0f,
                                           const AdamShadow* shadow = nullptr, float ema_d = 0.0f) {
    int ti = 0;
    while (ti + 1 < ts.count && (int)blockIdx.x >= ts.first_block[ti + 1]) ++ti;
    const long long base = (long long)((int)blockIdx.x - ts.first_block[ti]) * SIR_ADAM_CHUNK;
    float* __restrict__ p = ts.p[ti];
    const float* __restrict__ g = ts.g[ti];
    float* __restrict__ m = ts.m[ti];
    float* __restrict__ v = ts.v[ti];
    const long long n = ts.n[ti];
    const float step_size = lr / bc1;
#pragma unroll 4
    for (int k = 0; k < SIR_ADAM_CHUNK / 256; ++k) {
        const long long i = base + threadIdx.x + 256 * k;
        if (i >= n) break;
        float gi = g[i];
        if constexpr (CLIP) gi = __fmul_rn(gi, coef);
        float pi = p[i];
        if constexpr (DECOUPLED) pi = __fmul_rn(pi, decay_f);
        else if (weight_decay != 0.0f) gi = fmaf(weight_decay, pi, gi);
        const float mi = beta1 * m[i] + (1.0f - beta1) * gi;
        const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        const float pn = pi - step_size * (mi / denom);
        p[i] = pn;
        if constexpr (EMA) {
            float* __restrict__ e = shadow->e[ti];
            e[i] = fmaf(ema_d, e[i], __fmul_rn(1.0f - ema_d, pn));
        }
    }
}

static __global__ __launch_bounds__(256) void adam_multi_kernel(AdamTensors ts, float lr, float beta1, float beta2, float eps,
                                                          float weight_decay, float bc1, float bc2_sqrt) {
    adam_chunk<false>(ts, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, 1.0f);
}

// ------------------------------------------------------------------------------------------
// global gradient norm and clipping (torch.nn.utils.clip_grad_norm_, norm_type 2, error_if_nonfinite=False).
// Launch 1 leaves one fp32 sum of squares per 4096-element chunk (the block <-> chunk map of adam_multi_kernel) in a slab;
// whoever needs the norm sums the slab IN INDEX ORDER IN DOUBLE, so every block of every launch forms the same bits:
// no atomics, no last-block election ("What the profile says", item 4a).
// Summation tree of one partial: per thread a chain of 16 fmas (elements threadIdx.x + 256 k), then a binary tree of depth 8
// over the 256 threads in LDS.
// ------------------------------------------------------------------------------------------
struct GradTensors {
    float* g[SIR_ADAM_MAX_TENSORS];
    long long n[SIR_ADAM_MAX_TENSORS];
    int first_block[SIR_ADAM_MAX_TENSORS + 1];
    int count;
};

static __global__ __launch_bounds__(256) void grad_sumsq_kernel(GradTensors ts, float* __restrict__ partials) {
    __shared__ float red[256];
    int ti = 0;
    while (ti + 1 < ts.count && (int)blockIdx.x >= ts.first_block[ti + 1]) ++ti;
    const long long base = (long long)((int)blockIdx.x - ts.first_block[ti]) * SIR_ADAM_CHUNK;
    const float* __restrict__ g = ts.g[ti];
    const long long n = ts.n[ti];
    float v[SIR_ADAM_CHUNK / 256];
#pragma unroll
    for (int k = 0; k < SIR_ADAM_CHUNK / 256; ++k) {             // all 16 loads in flight; past the end: +0, which adds nothing
        const long long i = base + threadIdx.x + 256 * k;
        v[k] = i < n ? g[i] : 0.0f;
    }
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < SIR_ADAM_CHUNK / 256; ++k) acc = fmaf(v[k], v[k], acc);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

// {total_norm, coef} from the slab: thread 0 sums in index order in double, the block gets both through LDS.
// coef = min(1, max_norm / (total_norm + 1e-6)) in fp32 as torch forms it; a NaN stays a NaN (torch.clamp), an infinite norm
// gives coef 0 (and 0 * Inf = NaN in the gradient that caused it), as clip_grad_norm_ with error_if_nonfinite=False.
__device__ __forceinline__ float2 grad_norm_coef(const float* __restrict__ partials, int n_partials, float max_norm) {
    __shared__ float2 nc;
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll 8
        for (int i = 0; i < n_partials; ++i) s += (double)partials[i];
        const float total = (float)sqrt(s);
        const float c = max_norm / (total + 1e-6f);
        nc = make_float2(total, c > 1.0f ? 1.0f : c);
    }
    __syncthreads();
    return nc;
}

static __global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const float* __restrict__ partials, int n_partials,
                                                                  float max_norm, float* __restrict__ out2) {
    const float2 nc = grad_norm_coef(partials, n_partials, max_norm);
    if (threadIdx.x == 0) { out2[0] = nc.x; out2[1] = nc.y; }
}

// clip_grad_norm_'s in-place scale: same grid as launch 1, g *= coef (always multiplied, as torch does: coef == 1 leaves the bits)
static __global__ __launch_bounds__(256) void grad_scale_kernel(GradTensors ts, const float* __restrict__ partials, int n_partials,
                                                          float max_norm, float* __restrict__ out2) {
    const float2 nc = grad_norm_coef(partials, n_partials, max_norm);
    if (blockIdx.x == 0 && threadIdx.x == 0) { out2[0] = nc.x; out2[1] = nc.y; }
    int ti = 0;
    while (ti + 1 < ts.count && (int)blockIdx.x >= ts.first_block[ti + 1]) ++ti;
    const long long base = (long long)((int)blockIdx.x - ts.first_block[ti]) * SIR_ADAM_CHUNK;
    float* __restrict__ g = ts.g[ti];
    const long long n = ts.n[ti];
#pragma unroll 4
    for (int k = 0; k < SIR_ADAM_CHUNK / 256; ++k) {
        const long long i = base + threadIdx.x + 256 * k;
        if (i >= n) break;
        g[i] = __fmul_rn(g[i], nc.y);
    }
}

static __global__ __launch_bounds__(256) void adam_multi_clipped_kernel(AdamTensors ts, float lr, float beta1, float beta2, float eps,
                                                                  float weight_decay, float bc1, float bc2_sqrt,
                                                                  const float* __restrict__ partials, int n_partials,
                                                                  float max_norm, float* __restrict__ out2) {
    const float2 nc = grad_norm_coef(partials, n_partials, max_norm);
    if (blockIdx.x == 0 && threadIdx.x == 0) { out2[0] = nc.x; out2[1] = nc.y; }
    adam_chunk<true>(ts, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, nc.y);
}

// sir_adam_step_ex with decoupled weight decay and / or the EMA shadow on (with both off the host launches the two kernels
// above): same grid, same chunk map; CLIP as adam_multi_clipped_kernel, otherwise `partials` / `out2` are not read
template <bool CLIP, bool DECOUPLED, bool EMA>
static __global__ __launch_bounds__(256) void adam_multi_ex_kernel(AdamTensors ts, AdamShadow shadow, float lr, float beta1, float beta2,
                                                             float eps, float weight_decay, float decay_f, float ema_d, float bc1,
                                                             float bc2_sqrt, const float* __restrict__ partials, int n_partials,
                                                             float max_norm, float* __restrict__ out2) {
    float coef = 1.0f;
    if constexpr (CLIP) {
        const float2 nc = grad_norm_coef(partials, n_partials, max_norm);
        if (blockIdx.x == 0 && threadIdx.x == 0) { out2[0] = nc.x; out2[1] = nc.y; }
        coef = nc.y;
    }
    adam_chunk<CLIP, DECOUPLED, EMA>(ts, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, coef, decay_f, &shadow, ema_d);
}
