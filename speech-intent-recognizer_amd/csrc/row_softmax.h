// The softmax of one logit segment in one wave, shared by everything that reads a row after the forward pass: classification,
// evaluation and the temperature fit (evaluate.hip) and the joint decoder of the slot heads (slots_decode.hip).  One copy, so a
// quantity two calls both promise -- a slot's log-probability terms -- carries the same bits in both.
#pragma once
#include <cmath>
#include "sir_internal.h"
#include "wave_fft.h"      // wave_sum, wave_fence

namespace {

constexpr int kClsWaves = 4;                         // rows (= waves) per workgroup of the classify / decode kernels
constexpr int kMaxRows = 1 << 30;                    // rows per call: row indices and their grid strides stay far inside an int

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
    return x;
}
__device__ __forceinline__ bool is_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// One row in one wave.  l: this lane's logit (lanes >= C hold 0 and take no part).  The row maximum is subtracted BEFORE the
// scaling: d = (l - max l) * beta is one rounding of an (almost always exact) difference, so a small gap keeps its relative
// precision whatever the magnitude of the logits and of beta; l * beta - max(l * beta) would carry the absolute rounding of
// the two products.
struct RowSoftmax {
    float d, e;             // (l - max l) * beta <= 0, exp(d) (0 on lanes >= C)
    float rest, den;        // sum of e without the first maximum's exact 1, and 1 + rest: log(den) = log1pf(rest) keeps the small
                            // tail of a confident row that 1 + rest rounds away
    int rank;               // of this lane's class (meaningless on lanes >= C and on non-finite rows)
    bool finite;            // wave-uniform
};

__device__ __forceinline__ RowSoftmax row_softmax(float l, int lane, int C, float beta) {
    RowSoftmax r;
    const bool on = lane < C;
    r.finite = __ballot(on && is_nonfinite(l)) == 0ull;
    const float m = wave_max(on ? l : -INFINITY);
    r.d = (l - m) * beta;
    r.e = on ? expf(r.d) : 0.0f;
    const unsigned long long at_max = __ballot(on && l == m);
    const int first = at_max ? __ffsll((long long)at_max) - 1 : -1;                     // (no lane on a NaN row)
    r.rest = wave_sum(lane == first ? 0.0f : r.e);
    r.den = 1.0f + r.rest;
    int rank = 0;
    for (int j = 0; j < C; ++j) {
        const float lj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(l), j));
        rank += (lj > l || (lj == l && j < lane)) ? 1 : 0;
    }
    r.rank = rank;
    return r;
}

inline int classify_blocks(int batch) {
    const int b = (batch + kClsWaves - 1) / kClsWaves;
    return b > 4096 ? 4096 : b;
}

}  // namespace
