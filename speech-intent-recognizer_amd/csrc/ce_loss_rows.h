// Cross-entropy over one softmax segment of a logit row, for a workgroup of 256 threads: the row arithmetic, the valid-row
// count and the LDS sum that ce_loss_kernel (train_loss_optim_kernels.h, a single head) and ce_loss_slots_kernel (slots.hip,
// once per slot) both run.  The two differ in addressing alone -- a row's segment is logits + b * row_stride + start, C wide,
// and its label labels[b * label_stride + label_col]; a single head is (C, 0, 1, 0) -- so a slot's loss and gradient carry the
// bits of the single-head call on a contiguous copy of the segment (include/sir_hip.h) because they are the same statements.
//
// loss_b = -log softmax(l_b)[y_b]; dlogits = (softmax - onehot) * grad_scale / nvalid       (nn.CrossEntropyLoss(), train.py:242)
// SOFT: the target of row b is q = (1 - eps) (lam e[ya] + (1 - lam) e[yb]) + eps / C instead of e[ya] (mixup's two labels and
// label smoothing); loss_b = -sum_c q[c] log softmax[c] = log(den) - sum_c q[c] (l[c] - max) because sum q = 1,
// dlogits = softmax - q.  SOFT = false reads none of `labels_b`, `lam` and `eps`.
#pragma once
#include "sir_internal.h"

// Rows whose label is not ignore_index, on every thread.  nn.CrossEntropyLoss() has ignore_index = -100 by default: such a row
// contributes neither loss nor gradient and the mean is taken over the remaining rows (all rows ignored: 0 / 0 = NaN, as torch).
// cnt: 256 ints of LDS, free again after the caller's next barrier.
__device__ __forceinline__ float ce_valid_rows(const long long* __restrict__ labels, int B, int label_stride, int label_col, int* cnt) {
    int nv = 0;
    for (int b = threadIdx.x; b < B; b += 256) nv += labels[(size_t)b * label_stride + label_col] != -100ll ? 1 : 0;
    cnt[threadIdx.x] = nv;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) cnt[threadIdx.x] += cnt[threadIdx.x + o];
        __syncthreads();
    }
    return (float)cnt[0];
}

// The 256 threads' partials added in a fixed tree; the sum on every thread.  red: 256 floats of LDS, as cnt above.
__device__ __forceinline__ float ce_block_sum(float acc, float* red) {
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// This thread's rows (b = threadIdx.x, + 256, ...) of one segment -> its partial of the segment's loss sum; writes the segment's
// part of dlogits (row stride as logits) unless that is NULL.  C <= CMAX, the caller's choice between 32 and 64.
template <int CMAX, bool SOFT>
__device__ __forceinline__ float ce_rows(const float* __restrict__ logits, const long long* __restrict__ labels,
                                         const long long* __restrict__ labels_b, const float* __restrict__ lam, float eps,
                                         int B, int row_stride, int start, int label_stride, int label_col, int C, float nvalid,
                                         float grad_scale, float* __restrict__ dlogits, unsigned int* status) {
    float acc = 0.0f;
    for (int b = threadIdx.x; b < B; b += 256) {
        // the row goes into registers with ALL its loads in flight (C <= CMAX): the per-class loops of the first version waited
        // for one dependent load after the other, 15 us for 256 x 31 logits
        const float* r = logits + (size_t)b * row_stride + start;
        // any OTHER label outside [0, C) (nn.CrossEntropyLoss raises on it; train.py:242): flag the handle's status word
        // (SIR_EINVAL at the next sir_check_status) and make the loss NaN instead of reading out of bounds
        const long long yl = labels[(size_t)b * label_stride + label_col];
        const bool ignored = yl == -100ll;
        const bool bad = !ignored && (yl < 0 || yl >= (long long)C);
        if (bad) __hip_atomic_fetch_or(status, SIR_STATUS_CE_LABEL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int y = (bad || ignored) ? 0 : (int)yl;
        if constexpr (SOFT) {
            // the second label of an ignored row is not read; a bad one is flagged like a bad first label
            const long long yl2 = (labels_b && !ignored) ? labels_b[(size_t)b * label_stride + label_col] : yl;
            const bool bad2 = !ignored && (yl2 < 0 || yl2 >= (long long)C);
            if (bad2) __hip_atomic_fetch_or(status, SIR_STATUS_CE_LABEL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int y2 = (bad2 || ignored) ? 0 : (int)yl2;
            const float lm = (labels_b && lam) ? lam[b] : 1.0f;
            const float wa = (1.0f - eps) * lm, wb = (1.0f - eps) * (1.0f - lm), u = eps / (float)C;
            float v[CMAX];
#pragma unroll
            for (int c = 0; c < CMAX; ++c) v[c] = c < C ? r[c] : 0.0f;
            const float ra = r[y], rb = r[y2];
            float mx = v[0];
#pragma unroll
            for (int c = 1; c < CMAX; ++c) if (c < C) mx = fmaxf(mx, v[c]);
            float den = 0.0f, dsum = 0.0f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) if (c < C) { const float d = v[c] - mx; dsum += d; v[c] = expf(d); den += v[c]; }
            const float row = logf(den) - (wa * (ra - mx) + wb * (rb - mx) + u * dsum);
            acc += (bad || bad2) ? __builtin_nanf("") : (ignored ? 0.0f : row);
            if (dlogits) {
                const float inv = 1.0f / den, gs = ignored ? 0.0f : grad_scale / nvalid;
                float* dr = dlogits + (size_t)b * row_stride + start;
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    if (c < C) {
                        const float q = u + (c == y ? wa : 0.0f) + (c == y2 ? wb : 0.0f);
                        dr[c] = ignored ? 0.0f : (v[c] * inv - q) * gs;
                    }
            }
            continue;
        }
        float v[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) v[c] = c < C ? r[c] : 0.0f;
        const float ry = r[y];
        float mx = v[0];
#pragma unroll
        for (int c = 1; c < CMAX; ++c) if (c < C) mx = fmaxf(mx, v[c]);
        float den = 0.0f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) if (c < C) { v[c] = expf(v[c] - mx); den += v[c]; }
        const float lse = mx + logf(den);
        acc += bad ? __builtin_nanf("") : (ignored ? 0.0f : lse - ry);
        if (dlogits) {
            const float inv = 1.0f / den, gs = ignored ? 0.0f : grad_scale / nvalid;
            float* dr = dlogits + (size_t)b * row_stride + start;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) dr[c] = ignored ? 0.0f : (v[c] * inv - (c == y ? 1.0f : 0.0f)) * gs;
        }
    }
    return acc;
}
