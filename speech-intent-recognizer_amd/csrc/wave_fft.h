// In-wave FFT primitives: packed complex arithmetic, the 8-point butterfly, the two LDS exchange layouts of the 512-point transform
// that runs inside ONE wave (three radix-8 passes, two exchanges through the wave's private LDS slab, no workgroup barrier), and the
// wave reduction.  The one definition for the feature kernels (feat_common.h) and the reverb kernel (reverb.hip); each keeps its own
// fft512 over these -- features with LDS twiddles and single-b64 exchange reads, reverb with register twiddles and plain reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int XS = 72;           // first exchange: row stride (complex) -- conflict-free 64-bank ds_read_b64 in pass 2
constexpr int XS2 = 68;          // second exchange: row stride (complex), with the XOR swizzle of ex2_index

// Complex values are 2-vectors so that every complex add / sub / scale is ONE packed instruction (v_pk_add_f32,
// v_pk_mul_f32, v_pk_fma_f32 with op_sel / neg modifiers for the swaps and sign flips): a VALU instruction costs the same
// ~4 issue cycles whether it carries one float or two per lane, and the feature kernel is issue-bound (PMC: SQ_ACTIVE_INST_ANY
// = the kernel's duration at 4.3 cycles per instruction).
typedef float cf32 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ cf32 CF(float2 a) { return cf32{a.x, a.y}; }
__device__ __forceinline__ cf32 swp(cf32 a) { return __builtin_shufflevector(a, a, 1, 0); }
__device__ __forceinline__ cf32 mul_mi(cf32 a) { return cf32{a.y, -a.x}; }                       // a * (-i)
__device__ __forceinline__ cf32 cmul(cf32 a, cf32 b) {                                           // a * b
    return cf32{a.x, a.x} * b + cf32{a.y, a.y} * cf32{-b.y, b.x};
}

// slot of element (row k2, j, m1) in the second exchange: (j, m1) -> (j ^ (m1 >> 1)) + 8 m1 is injective, the 16 lanes
// (k2 in {2g, 2g+1}, m1) of a ds_write_b64 group land on 16 different bank pairs mod 32, and the 32 lanes (k2, j2 in
// {4g .. 4g+3}) of a ds_read_b64 group on 32 different bank pairs mod 64 (row stride 68: 136 words = 8 mod 64)
__device__ __forceinline__ int ex2_index(int k2, int j, int m1) { return k2 * XS2 + ((j ^ (m1 >> 1)) + 8 * m1); }

// Eight single ds_read_b64 + their wait in ONE asm statement (cdna_hip_programming.md 5.7 form (i)): hipcc pairs plain --
// and volatile -- adjacent LDS loads into ds_read2_b64 / ds_read2st64_b64, which move half the bytes per LDS cycle.
typedef cf32 f32x2;
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(uintptr_t)p; }   // LDS byte offset of a __shared__ pointer

// v[m] = *(base + m * STRIDE_BYTES), m = 0..7
template <int STRIDE_BYTES>
__device__ __forceinline__ void lds_read8(unsigned base, cf32 (&v)[8]) {
    f32x2 r0, r1, r2, r3, r4, r5, r6, r7;
    asm volatile(
        "ds_read_b64 %0, %8 offset:%9\n\tds_read_b64 %1, %8 offset:%10\n\tds_read_b64 %2, %8 offset:%11\n\t"
        "ds_read_b64 %3, %8 offset:%12\n\tds_read_b64 %4, %8 offset:%13\n\tds_read_b64 %5, %8 offset:%14\n\t"
        "ds_read_b64 %6, %8 offset:%15\n\tds_read_b64 %7, %8 offset:%16\n\ts_waitcnt lgkmcnt(0)"
        : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7)
        : "v"(base), "i"(0 * STRIDE_BYTES), "i"(1 * STRIDE_BYTES), "i"(2 * STRIDE_BYTES), "i"(3 * STRIDE_BYTES),
          "i"(4 * STRIDE_BYTES), "i"(5 * STRIDE_BYTES), "i"(6 * STRIDE_BYTES), "i"(7 * STRIDE_BYTES)
        : "memory");
    v[0] = r0; v[1] = r1; v[2] = r2; v[3] = r3; v[4] = r4; v[5] = r5; v[6] = r6; v[7] = r7;
}
// v[m] = *(base[m >> 1] + m * STRIDE_BYTES): the XOR-swizzled second exchange (one base per value of m >> 1)
template <int STRIDE_BYTES>
__device__ __forceinline__ void lds_read8x4(unsigned b0, unsigned b1, unsigned b2, unsigned b3, cf32 (&v)[8]) {
    f32x2 r0, r1, r2, r3, r4, r5, r6, r7;
    asm volatile(
        "ds_read_b64 %0, %8 offset:%12\n\tds_read_b64 %1, %8 offset:%13\n\tds_read_b64 %2, %9 offset:%14\n\t"
        "ds_read_b64 %3, %9 offset:%15\n\tds_read_b64 %4, %10 offset:%16\n\tds_read_b64 %5, %10 offset:%17\n\t"
        "ds_read_b64 %6, %11 offset:%18\n\tds_read_b64 %7, %11 offset:%19\n\ts_waitcnt lgkmcnt(0)"
        : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7)
        : "v"(b0), "v"(b1), "v"(b2), "v"(b3), "i"(0 * STRIDE_BYTES), "i"(1 * STRIDE_BYTES), "i"(2 * STRIDE_BYTES),
          "i"(3 * STRIDE_BYTES), "i"(4 * STRIDE_BYTES), "i"(5 * STRIDE_BYTES), "i"(6 * STRIDE_BYTES), "i"(7 * STRIDE_BYTES)
        : "memory");
    v[0] = r0; v[1] = r1; v[2] = r2; v[3] = r3; v[4] = r4; v[5] = r5; v[6] = r6; v[7] = r7;
}

// forward 8-point DFT, natural order in and out (decimation in frequency)
__device__ __forceinline__ void dft8(cf32 (&v)[8]) {
    const float R = 0.70710678118654752440f;
    cf32 a0 = v[0] + v[4], a4 = v[0] - v[4];
    cf32 a1 = v[1] + v[5], a5 = v[1] - v[5];
    cf32 a2 = v[2] + v[6], a6 = v[2] - v[6];
    cf32 a3 = v[3] + v[7], a7 = v[3] - v[7];
    a5 = (a5 + mul_mi(a5)) * R;                                  // * W8^1 = (x + y, y - x) / sqrt 2
    a6 = mul_mi(a6);                                             // * W8^2
    a7 = (mul_mi(a7) - a7) * R;                                  // * W8^3 = (y - x, -x - y) / sqrt 2
    cf32 b0 = a0 + a2, b2 = a0 - a2, b1 = a1 + a3, b3 = mul_mi(a1 - a3);
    cf32 c0 = a4 + a6, c2 = a4 - a6, c1 = a5 + a7, c3 = mul_mi(a5 - a7);
    v[0] = b0 + b1; v[4] = b0 - b1; v[2] = b2 + b3; v[6] = b2 - b3;
    v[1] = c0 + c1; v[5] = c0 - c1; v[3] = c2 + c3; v[7] = c2 - c3;
}

__device__ __forceinline__ void wave_fence() {
    // per-wave LDS slab: LDS ops of one wave execute in order, only the compiler must not reorder
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace
