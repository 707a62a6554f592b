// The two-way fp16 split of an fp32 value ("f16x3" contractions, f16x3_kernels.h):
//     hi = fp16(x)  (round to nearest, 11 significant bits)         lo = fp16((x - hi) * 2^11)
// x - hi is exact in fp32; the residual is scaled by 2^11 so that it sits in fp16's normal range wherever hi does.
// hi + lo * 2^-11 carries 22-23 significant bits of x for 2^-14 <= |x| <= 65504; smaller values keep an ABSOLUTE error of
// 2^-36 (the backward keeps its operands above that by choosing its loss scale from the gradients it is handed: train_workspace.h).
// Values beyond fp16's range are clamped to +-65504 first (an overflow to infinity would turn 0 * inf products into NaNs), and
// the clamp (fminf / fmaxf) turns a NaN into a finite number too: nothing non-finite survives a split.  Where that could hide a
// fault from the caller it is reported instead -- weights by the preparation kernels (split_flag_range below, split_w_f16x3),
// features by the scans that read them anyway (include/sir_hip.h at sir_model_infer has the whole contract).
#pragma once

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 sir_f16x2 __attribute__((ext_vector_type(2)));

constexpr float H3_LO_SCALE = 2048.0f;                      // 2^11
constexpr float H3_LO_INV = 1.0f / 2048.0f;

// two floats -> packed hi halves, packed scaled-residual halves (a in the low 16 bits)
__device__ __forceinline__ void split2h_pair(float a, float b, unsigned& h, unsigned& l) {
    sir_f32x2 v = {__builtin_fminf(__builtin_fmaxf(a, -65504.0f), 65504.0f), __builtin_fminf(__builtin_fmaxf(b, -65504.0f), 65504.0f)};
    const sir_f16x2 hi = __builtin_convertvector(v, sir_f16x2);
    v -= __builtin_convertvector(hi, sir_f32x2);            // exact
    v *= H3_LO_SCALE;
    const sir_f16x2 lo = __builtin_convertvector(v, sir_f16x2);
    h = __builtin_bit_cast(unsigned, hi);
    l = __builtin_bit_cast(unsigned, lo);
}
// the same without the clamps, for waves that run with MODE.FP16_OVFL = 1 (an overflowing conversion then saturates at +-65504 by itself)
__device__ __forceinline__ void split2h_pair_ovfl(float a, float b, unsigned& h, unsigned& l) {
    // (lo' as one v_fma_mixlo / mixhi_f16 per value -- 4 instead of 6 instructions per pair, the same rounding -- was measured: no faster)
    sir_f32x2 v = {a, b};
    const sir_f16x2 hi = __builtin_convertvector(v, sir_f16x2);
    v -= __builtin_convertvector(hi, sir_f32x2);
    v *= H3_LO_SCALE;
    const sir_f16x2 lo = __builtin_convertvector(v, sir_f16x2);
    h = __builtin_bit_cast(unsigned, hi);
    l = __builtin_bit_cast(unsigned, lo);
}
__device__ __forceinline__ void split2h_quad_ovfl(const float4& v, uint2& h, uint2& l) {
    split2h_pair_ovfl(v.x, v.y, h.x, l.x);
    split2h_pair_ovfl(v.z, v.w, h.y, l.y);
}
// MODE.FP16_OVFL = 1 for the calling wave (hwreg id 1 = MODE, bit 23): fp16 results that overflow saturate at +-65504 instead of becoming infinity
__device__ __forceinline__ void sir_fp16_ovfl_on() { __builtin_amdgcn_s_setreg(1 | (23 << 6) | (0 << 11), 1); }
__device__ __forceinline__ void split2h_quad(const float4& v, uint2& h, uint2& l) {
    split2h_pair(v.x, v.y, h.x, l.x);
    split2h_pair(v.z, v.w, h.y, l.y);
}

// Weight preparation only: a GRU matrix element the split would clamp (|w| > 65504) or that is not finite -- the clamp turns a NaN into
// a finite number -- raises bit 11 of the handle's status word (SIR_EINVAL at the next sir_check_status).  status == NULL: no check.
__device__ __forceinline__ void split_flag_range(const float4& a, const float4& b, unsigned int* status) {
    if (!status) return;
    const bool ok = fabsf(a.x) <= 65504.0f && fabsf(a.y) <= 65504.0f && fabsf(a.z) <= 65504.0f && fabsf(a.w) <= 65504.0f &&
                    fabsf(b.x) <= 65504.0f && fabsf(b.y) <= 65504.0f && fabsf(b.z) <= 65504.0f && fabsf(b.w) <= 65504.0f;
    if (!ok) __hip_atomic_fetch_or(status, SIR_STATUS_GRU_WEIGHT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// in [rows][K] fp32 (row stride ld_in) -> planes [2][rows][K] fp16; one thread = 8 consecutive k.  status: split_flag_range (weights)
__device__ __forceinline__ void split2h_rows(const float* __restrict__ in, int ld_in, unsigned short* __restrict__ out, size_t rows, int K,
                                             size_t gidx, size_t nthreads, unsigned int* status = nullptr) {
    const int k8n = K / 8;
    const size_t total = rows * k8n, plane = rows * (size_t)K;
    for (size_t idx = gidx; idx < total; idx += nthreads) {
        const size_t row = idx / k8n;
        const int k8 = idx % k8n;
        const float4 v0 = *reinterpret_cast<const float4*>(in + row * ld_in + k8 * 8);
        const float4 v1 = *reinterpret_cast<const float4*>(in + row * ld_in + k8 * 8 + 4);
        uint2 h0, l0, h1, l1;
        split_flag_range(v0, v1, status);
        split2h_quad(v0, h0, l0);
        split2h_quad(v1, h1, l1);
        const size_t o = row * K + (size_t)k8 * 8;
        *reinterpret_cast<uint4*>(out + o) = make_uint4(h0.x, h0.y, h1.x, h1.y);
        *reinterpret_cast<uint4*>(out + plane + o) = make_uint4(l0.x, l0.y, l1.x, l1.y);
    }
}
#ifndef SIR_NO_STANDALONE_KERNELS
static __global__ __launch_bounds__(256) void split2h_kernel(const float* __restrict__ in, int ld_in, unsigned short* __restrict__ out,
                                                              size_t rows, int K) {
    split2h_rows(in, ld_in, out, rows, K, (size_t)blockIdx.x * 256 + threadIdx.x, (size_t)gridDim.x * 256);
}
// the same for a weight matrix (inference prepares W_ih with it): out-of-range / non-finite elements are reported
static __global__ __launch_bounds__(256) void split2h_weights_kernel(const float* __restrict__ in, int ld_in, unsigned short* __restrict__ out,
                                                                      size_t rows, int K, unsigned int* status) {
    split2h_rows(in, ld_in, out, rows, K, (size_t)blockIdx.x * 256 + threadIdx.x, (size_t)gridDim.x * 256, status);
}
#endif
