// A 512-float row read by one wave, its norm and its unit vector: the code sir_proto_accumulate, sir_proto_score (prototypes.hip)
// and sir_proxy_loss (proxy_loss.hip) share, so that a row's unit vector carries the same bits in all of them.
// ONE WAVE OWNS A ROW, lane l holds its elements 8 l .. 8 l + 7 (two 16-byte loads).  The sum of squares is formed in double --
// the lane's eight squares in element order, then the xor butterfly over the 64 lanes (32, 16, ... 1: every lane ends with the
// same bits) -- so it depends on nothing but the row, and so does e / sqrt(sumsq), the quotient taken in double.
#pragma once
#include "sir_internal.h"
#include "row_softmax.h"   // is_nonfinite

namespace {

constexpr int kDim = 512;                            // floats of an embedding
constexpr int kMaxProtos = 4096;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the lane's eight elements of a 512-float row (16-byte aligned)
__device__ __forceinline__ void load_row8(const float* __restrict__ row, int lane, float (&e)[8]) {
    const float4 a = reinterpret_cast<const float4*>(row)[2 * lane], b = reinterpret_cast<const float4*>(row)[2 * lane + 1];
    e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w; e[4] = b.x; e[5] = b.y; e[6] = b.z; e[7] = b.w;
}

// One row in one wave: false (wave-uniform) for a row with a NaN or an infinity or with norm zero; else norm = ||e|| in double.
// The sum of squares: the lane's eight squares in element order, then the butterfly -- a function of the row alone.
__device__ __forceinline__ bool row_norm(const float (&e)[8], double& norm) {
#pragma clang fp contract(off)
    bool bad = false;
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        bad = bad || is_nonfinite(e[i]);
        const double x = (double)e[i];
        ss += x * x;
    }
    ss = wave_sum_f64(ss);
    const bool ok = __ballot(bad) == 0ull && ss > 0.0;
    norm = ok ? sqrt(ss) : 1.0;
    return ok;
}
// element i of the unit vector, in double: e / ||e|| as e * (1 / ||e||) would round twice -- the quotient is taken directly
__device__ __forceinline__ double unit_elem(float e, double norm) { return (double)e / norm; }

}  // namespace
