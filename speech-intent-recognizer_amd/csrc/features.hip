// Fused feature kernel: waveform batch -> normalised, zero-padded log-mel [B][n_mels][t_pad], ONE launch.
//
// Replaces (per clip, on CPU, one at a time in the reference):
//   torchaudio MelSpectrogram + AmplitudeToDB + z-norm   scripts/precompute_features.py:59-73
//   pad/trim to 200 frames                                scripts/dataset.py:109-113
//   SpecAugment bands / time_shift / add_noise            scripts/dataset.py:160-176, scripts/augment.py:6-28, :82-96
//
// feat_utt_kernel: one workgroup of 16 waves owns ONE utterance and walks its frames 16 at a time ("rounds"):
//   * FFT: wave w transforms frame 16 r + w.  1024 real samples (reflect-padded, Hann-windowed on load, the next
//     round's samples already in flight) are packed into 512 complex points, 8 per lane, and run through three
//     radix-8 passes (register butterflies, two exchanges through the wave's private LDS slab -- no workgroup
//     barrier inside the transform), then untangled to the 513-bin power spectrum, written to row w of P.
//   * mel: after one barrier all 16 spectra of the round are in LDS and the 1024 threads split the 16 x 64
//     (frame, filter) dot products one each: a thread walks only ITS filter's taps (2 ... 41 of them; the
//     filterbank is stored compact), filters are sorted by length so the four filters a wave handles are equally
//     long, and lanes that read P differ in the frame (row stride 513 words: a different bank each).  This is
//     1000 multiply-adds per frame instead of the 64 x 41 padded ones of a lane-per-filter loop.
//   * log-compress: the thread keeps its dB value of every round IN A REGISTER (10 rounds = 160 frames; 5 s clips are
//     157 frames), so the utterance's whole [64 x T] dB tile lives in the register file.  After the last round the
//     workgroup reduces mean and unbiased variance over it (two passes, double-precision combine) and every thread
//     stores (x - mean) / (std + 1e-5) of its own values with the SpecAugment bands and the zero padding (64-byte row
//     segments): no second kernel, no statistics round trip through L2, no tile in LDS -- which leaves room to
//     double-buffer P, so a round costs ONE workgroup barrier.
//     Clips longer than 160 frames (only the single-file predict surface feeds those) park their dB values in the
//     output rows instead and the same workgroup re-reads them for the two passes (same CU, same L1: no
//     inter-workgroup visibility involved).
// LDS traffic is what bounds the transform (PMC: the LDS pipe was busy 45 % of the first fused version, 29 % of that
// bank conflicts), hence: every exchange read is a single ds_read_b64 (`volatile`: hipcc otherwise pairs them into
// ds_read2_b64, which moves HALF the bytes per LDS cycle and banks mod 32 in 16-lane groups); the second exchange uses a
// stride-68 XOR-swizzled layout that is conflict-free for its 16-lane ds_write_b64 groups AND its 32-lane ds_read_b64
// groups; the untangle partner Z[512-k] comes from lane (64 - lane) by ds_bpermute instead of a store + load.
// HBM traffic per utterance (algorithmic): L*4 B read (L*2 for PCM16) + n_mels*t_pad*4 B written.
// feat_utt_kernel is the front-end n_fft 1024 / hop 512 / win_length 1024 only; every other supported one runs the general launch
// pair further down (feat_gen_frames_kernel + feat_gen_norm_kernel).
#include <stdint.h>
#include "sir_internal.h"

namespace {

constexpr int NW = 16;           // waves per workgroup = frames per round
constexpr int THREADS = NW * 64;
constexpr int XS = 72;           // first exchange: row stride (complex) -- conflict-free 64-bank ds_read_b64 in pass 2
constexpr int XS2 = 68;          // second exchange: row stride (complex), with the XOR swizzle of ex2_index
constexpr int XBUF = 8 * XS;     // complex slots per wave
constexpr int PROW = 514;        // words per power-spectrum row: the 16 frames of a filter sit on 16 different banks
constexpr int TW2S = 10;         // row stride (complex) of the pass-2 twiddle table in LDS
constexpr int RMAX = 10;         // rounds whose dB values a thread keeps in registers
constexpr int TILE_T = RMAX * NW;   // = 160 frames
constexpr float AMIN = 1e-10f;
constexpr float NORM_EPS = 1e-5f;

struct FeatTables {
    const float2* tw512;
    const float2* tw1024;
    const float* window;
    const float* melw;           // compact filter weights, filter after filter, taps ascending in frequency
    const int4* mel_desc;        // [64] per SLOT (filters sorted by tap count): {filter, first bin, taps, offset into melw}
    int mel_nnz;
    int n_mels;
};

struct AugArgs {
    const int32_t* shift;
    const float* sigma;
    unsigned long long seed;
};

// Complex values are 2-vectors so that every complex add / sub / scale is ONE packed instruction (v_pk_add_f32,
// v_pk_mul_f32, v_pk_fma_f32 with op_sel / neg modifiers for the swaps and sign flips): a VALU instruction costs the same
// ~4 issue cycles whether it carries one float or two per lane, and this kernel is issue-bound (PMC: SQ_ACTIVE_INST_ANY
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

__device__ __forceinline__ unsigned fmix32(unsigned x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}
// Two independent standard normals, a pure function of (seed, utterance, sample PAIR index p): samples 2p and 2p+1 of the
// clip take .x and .y, so every frame that touches a sample sees the same noise value (Box-Muller on two 24-bit
// uniforms from a counter hash; hardware log2 / sqrt / sin / cos: ~1e-6 absolute, far below the sigma <= 1e-2 it scales).
// Restated on the host in tests/host_rng.py.
__device__ __forceinline__ float2 gauss_pair(unsigned long long seed, int b, int p) {
    const unsigned k = fmix32((unsigned)seed ^ ((unsigned)p * 0x9E3779B1u) ^ ((unsigned)b * 0x85EBCA77u));
    const unsigned a = fmix32(k ^ (unsigned)(seed >> 32));
    const unsigned c = fmix32(a + 0x632BE5ABu + (unsigned)p);
    const float u1 = (float)((a >> 8) + 1u) * (1.0f / 16777216.0f);      // (0, 1]
    const float u2 = (float)(c >> 8) * (1.0f / 16777216.0f);             // [0, 1)  (revolutions)
    const float r = __builtin_amdgcn_sqrtf(-1.38629436111989061883f * __builtin_amdgcn_logf(u1));   // sqrt(-2 ln u1), logf = log2
    return make_float2(r * __builtin_amdgcn_cosf(u2), r * __builtin_amdgcn_sinf(u2));
}

template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<short>(short v) { return (float)v * (1.0f / 32768.0f); }

// sample i of the (augmented) clip after reflect padding; needs L > 512
template <typename T, bool AUG>
__device__ __forceinline__ float fetch(const T* __restrict__ x, int L, int i, int shift, float sigma,
                                       unsigned long long seed, int b) {
    if (i < 0) i = -i;
    else if (i >= L) i = 2 * L - 2 - i;
    if (AUG) {
        int s = i - shift;
        float v = (s >= 0 && s < L) ? to_f32<T>(x[s]) : 0.0f;
        if (sigma > 0.0f) {
            const float2 g = gauss_pair(seed, b, i >> 1);
            v += sigma * ((i & 1) ? g.y : g.x);
        }
        return v;
    }
    return to_f32<T>(x[i]);
}

// the 16 samples of one lane for frame t (pairs (i0, i0 + 1), i0 = base + 2 (lane + 64 j)), un-windowed
template <typename T, bool AUG>
__device__ __forceinline__ void load_frame(const T* __restrict__ x, int L, int t, int lane, int shift, float sigma,
                                           unsigned long long seed, int b, cf32 (&s)[8]) {
    const int base = t * SIR_HOP - SIR_HOP;         // first padded sample of the frame, in clip coordinates
    const bool interior = base >= 0 && base + SIR_NFFT <= L;          // wave-uniform: no reflection in this frame
    const bool paired = (reinterpret_cast<uintptr_t>(x) & (2 * sizeof(T) - 1)) == 0;   // row starts on a sample-pair boundary
    if (interior && !AUG && !paired) {              // odd row stride / offset view: two scalar loads per pair
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const T* q = x + base + 2 * (lane + 64 * j);
            s[j] = cf32{to_f32<T>(q[0]), to_f32<T>(q[1])};
        }
        return;
    }
    if (interior && !AUG) {
        if (sizeof(T) == 4) {
            const cf32* p = reinterpret_cast<const cf32*>(x + base) + lane;           // base is even: 8-byte aligned rows
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = p[64 * j];
        } else {
            const unsigned* p = reinterpret_cast<const unsigned*>(x + base) + lane;   // two PCM16 samples per word
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned w = p[64 * j];
                s[j] = cf32{(float)(short)(w & 0xFFFFu), (float)(short)(w >> 16)} * (1.0f / 32768.0f);
            }
        }
        return;
    }
    if (interior && AUG) {                          // shifted reads + ONE noise pair per lane and j (i0 is even)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i0 = base + 2 * (lane + 64 * j), s0 = i0 - shift;
            cf32 v;
            v.x = (s0 >= 0 && s0 < L) ? to_f32<T>(x[s0]) : 0.0f;
            v.y = (s0 + 1 >= 0 && s0 + 1 < L) ? to_f32<T>(x[s0 + 1]) : 0.0f;
            if (sigma > 0.0f) {
                const float2 g = gauss_pair(seed, b, i0 >> 1);
                v += sigma * cf32{g.x, g.y};
            }
            s[j] = v;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {                   // first / last frames: reflect padding, element by element
        const int i0 = base + 2 * (lane + 64 * j);
        s[j].x = fetch<T, AUG>(x, L, i0, shift, sigma, seed, b);
        s[j].y = fetch<T, AUG>(x, L, i0 + 1, shift, sigma, seed, b);
    }
}

__device__ __forceinline__ void wave_fence() {
    // per-wave LDS slab: LDS ops of one wave execute in order, only the compiler must not reorder
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// 512-point complex DFT inside one wave: on entry lane holds points lane + 64 j, on return bins lane + 64 j (j = register).
// Three radix-8 passes with two exchanges through the wave's own slab xb -- feat_utt_kernel's transform, which keeps its own inline
// copy (and its pass-1 twiddles in registers); tw1col[64 k] = W512^(lane * k) in LDS, tw2row = row lane & 7 of the pass-2
// twiddle table, a_p2 / a_p3 = the lane's read columns of the two exchanges.  No workgroup barrier.
__device__ __forceinline__ void fft512(cf32 (&v)[8], const cf32* tw1col, const cf32* tw2row, cf32* xb, int lane,
                                       unsigned a_p2, const unsigned (&a_p3)[4]) {
    // pass 1: DFT over n2 (stride 64), twiddle W512^(n1*k2)
    dft8(v);
#pragma unroll
    for (int k = 1; k < 8; ++k) v[k] = cmul(v[k], tw1col[64 * k]);
    wave_fence();
#pragma unroll
    for (int k = 0; k < 8; ++k) xb[k * XS + lane] = v[k];
    wave_fence();
    {   // pass 2: lane = (k2, m1): DFT over m2, twiddle W64^(m1*j2)
        const int k2 = lane >> 3, m1p = lane & 7;
        lds_read8<8 * 8>(a_p2, v);              // xb[k2 * XS + m1p + 8 m]
        dft8(v);
#pragma unroll
        for (int k = 1; k < 8; ++k) v[k] = cmul(v[k], tw2row[k]);
        wave_fence();
#pragma unroll
        for (int j = 0; j < 8; ++j) xb[ex2_index(k2, j, m1p)] = v[j];
        wave_fence();
    }
    {   // pass 3: lane = k2 + 8*j2: DFT over m1 -> Z[lane + 64*j1]
        lds_read8x4<8 * 8>(a_p3[0], a_p3[1], a_p3[2], a_p3[3], v);   // xb[ex2_index(lane & 7, lane >> 3, m)]
        dft8(v);
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// workgroup sum of one float per thread, combined in double (deterministic order); every thread gets the result
__device__ __forceinline__ double block_sum(float v, double* red, int lane, int wv) {
    v = wave_sum(v);
    __syncthreads();                                 // red is reused across calls
    if (lane == 0) red[wv] = (double)v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) s += red[i];
    return s;
}

template <typename WT, bool AUG>
__global__ __launch_bounds__(THREADS) void feat_utt_kernel(
    const WT* __restrict__ wave, long long wave_stride, const int32_t* __restrict__ lengths, int max_len,
    float* __restrict__ out, float* __restrict__ db_out, int t_pad, FeatTables tb, AugArgs aug,
    const int32_t* __restrict__ time_mask, const int32_t* __restrict__ freq_mask) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cf32* xall = reinterpret_cast<cf32*>(smem);                        // [NW][XBUF] exchange slabs
    double* red = reinterpret_cast<double*>(xall + NW * XBUF);         // [NW] reduction scratch
    float* Pbuf = reinterpret_cast<float*>(red + NW);                  // [2][NW][PROW] power spectra, by round parity
    float* melw = Pbuf + 2 * NW * PROW;                                // [mel_nnz]
    cf32* winl = reinterpret_cast<cf32*>(melw + ((tb.mel_nnz + 3) & ~3));       // [512] Hann window as sample pairs
    cf32* twul = winl + 512;                                           // [512] -i/2 * W1024^k, the untangle twiddles
    cf32* tw2l = twul + 512;                                           // [8][TW2S] W64^(m1 * j2), row m1 (stride 10: the 8 rows' 16-byte reads fall on disjoint banks)

    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n_mels = tb.n_mels;
    int L = lengths[b];
    if (L > max_len) L = max_len;
    const int T = (L > SIR_HOP) ? 1 + L / SIR_HOP : 0;                 // L <= 512: the reference fails (reflect pad) -> zero row
    const int tv = T < t_pad ? T : t_pad;
    float* orow = out + (size_t)b * n_mels * t_pad;
    float* drow = db_out ? db_out + (size_t)b * n_mels * t_pad : nullptr;
    const bool in_regs = T <= TILE_T;                                  // block-uniform
    const int nrounds = (T + NW - 1) / NW;
    // mel role of this thread: (frame of the round, filter slot); the four slots of a wave are equally long filters
    const int mf = tid & 15;
    const int4 md = tb.mel_desc[tid >> 4];                             // {filter, first bin, taps, offset}
    float dbv[RMAX];                                                   // this thread's dB values: frame 16 r + mf of filter md.x
#pragma unroll
    for (int r = 0; r < RMAX; ++r) dbv[r] = 0.0f;

    if (nrounds > 0) {
        for (int i = tid; i < tb.mel_nnz; i += THREADS) melw[i] = tb.melw[i];
        if (tid < 512) {
            winl[tid] = reinterpret_cast<const cf32*>(tb.window)[tid];
            // X[k] = (z + conj zp)/2 + (-i/2 W1024^k)(z - conj zp)
            twul[tid] = 0.5f * mul_mi(CF(tb.tw1024[tid]));
        }
        if (tid < 64) tw2l[(tid >> 3) * TW2S + (tid & 7)] = CF(tb.tw512[(8 * (tid >> 3) * (tid & 7)) & 511]);

        // per-lane constants of the transform, reused for every frame of this wave (the window, the pass-2 twiddles -- which only
        // depend on lane & 7 -- and the untangle twiddles live in LDS: 46 more registers per lane would spill at four waves per SIMD)
        cf32 tw1[8];
        const int m1p = lane & 7;
#pragma unroll
        for (int k = 0; k < 8; ++k) tw1[k] = CF(tb.tw512[(lane * k) & 511]);        // W512^(n1*k2)
        const WT* x = wave + (size_t)b * wave_stride;
        int shift = 0;
        float sigma = 0.0f;
        if (AUG) {
            if (aug.shift) shift = aug.shift[b];
            if (aug.sigma) sigma = aug.sigma[b];
        }
        cf32* xb = xall + wv * XBUF;
        const int mirror = ((64 - lane) & 63) * 4;          // ds_bpermute address of the lane that holds Z[512 - k]
        // LDS byte addresses of this lane's read columns (loop-invariant)
        const unsigned a_win = lds_addr(winl + lane);
        const unsigned a_p2 = lds_addr(xb + (lane >> 3) * XS + m1p);
        unsigned a_p3[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) a_p3[q] = lds_addr(xb + (lane & 7) * XS2 + ((lane >> 3) ^ q));

        cf32 nxt[8];
        if (wv < T) load_frame<WT, AUG>(x, L, wv, lane, shift, sigma, aug.seed, b, nxt);
        __syncthreads();                                    // mel weights and window are staged

        for (int r = 0; r < nrounds; ++r) {
            const int t = r * NW + wv;
            float* P = Pbuf + (r & 1) * (NW * PROW);
            if (t < T) {                                    // wave-uniform
                cf32 v[8];
                lds_read8<64 * 8>(a_win, v);                // window pairs lane + 64 j
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = nxt[j] * v[j];       // (a product only: nothing to fuse)
                if (t + NW < T) load_frame<WT, AUG>(x, L, t + NW, lane, shift, sigma, aug.seed, b, nxt);   // next round's samples
                // pass 1: DFT over n2 (stride 64), twiddle W512^(n1*k2)
                dft8(v);
#pragma unroll
                for (int k = 1; k < 8; ++k) v[k] = cmul(v[k], tw1[k]);
                wave_fence();
#pragma unroll
                for (int k = 0; k < 8; ++k) xb[k * XS + lane] = v[k];
                wave_fence();
                {   // pass 2: lane = (k2, m1): DFT over m2, twiddle W64^(m1*j2)
                    const int k2 = lane >> 3;
                    lds_read8<8 * 8>(a_p2, v);              // xb[k2 * XS + m1p + 8 m]
                    dft8(v);
#pragma unroll
                    for (int k = 1; k < 8; ++k) v[k] = cmul(v[k], tw2l[TW2S * m1p + k]);
                    wave_fence();
#pragma unroll
                    for (int j = 0; j < 8; ++j) xb[ex2_index(k2, j, m1p)] = v[j];
                    wave_fence();
                }
                {   // pass 3: lane = k2 + 8*j2: DFT over m1 -> Z[lane + 64*j1]
                    lds_read8x4<8 * 8>(a_p3[0], a_p3[1], a_p3[2], a_p3[3], v);   // xb[ex2_index(lane & 7, lane >> 3, m)]
                    dft8(v);
                }
                // untangle the packed real transform: X[k] = (z + conj zp)/2 + (-i/2 W1024^k)(z - conj zp), power = |X|^2,
                // k = lane + 64 j.  The partner zp = Z[512 - k] is register 7 - j of lane 64 - lane (lane 0: its own
                // register 8 - j, and Z[512] = Z[0]).
                float* prow = P + wv * PROW;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const cf32 z = v[j];
                    cf32 zc;
                    zc.x = __int_as_float(__builtin_amdgcn_ds_bpermute(mirror, __float_as_int(v[7 - j].x)));
                    zc.y = __int_as_float(__builtin_amdgcn_ds_bpermute(mirror, __float_as_int(v[7 - j].y)));
                    if (lane == 0) zc = v[(8 - j) & 7];
                    zc.y = -zc.y;                           // conj(zp)
                    const cf32 xk = 0.5f * (z + zc) + cmul(z - zc, twul[lane + 64 * j]);
                    const cf32 sq = xk * xk;
                    prow[lane + 64 * j] = sq.x + sq.y;
                }
                if (lane == 0) { const float n = v[0].x - v[0].y; prow[512] = n * n; }       // X[512] = Re Z0 - Im Z0
            }
            __syncthreads();                                // all spectra of this round are in P (the other parity is free again)
            // sparse HTK mel filterbank: thread = (frame mf, filter md.x), taps ascending in frequency
            const int tm = r * NW + mf;
            if (md.x >= 0 && tm < T) {
                const float* pr = P + mf * PROW + md.y;
                const float* wr = melw + md.w;
                float acc = 0.0f;
                for (int i = 0; i < md.z; ++i) acc = fmaf(wr[i], pr[i], acc);
                // the 1e-10 clamp is exact in the reference (silence -> exactly -100 dB)
                const float db = (acc <= AMIN) ? -100.0f : 10.0f * log10f(acc);
                if (in_regs) {
#pragma unroll
                    for (int q = 0; q < RMAX; ++q) dbv[q] = (q == r) ? db : dbv[q];
                } else if (tm < t_pad) {
                    orow[(size_t)md.x * t_pad + tm] = db;   // long clip: dB parked in the output row
                }
            }
        }
        __syncthreads();
    }

    // ---- whole-utterance statistics (two passes) and the normalised, masked, zero-padded store ----------------------
    // the statistics are over ALL frames of the clip (precompute_features.py:73 normalises before any trim); a clip
    // longer than 160 frames has every frame parked in its output row (the host checks t_pad >= T for those)
    float mean = 0.0f, denom = 1.0f;
    const bool mine = md.x >= 0;
    if (T > 0) {
        float s = 0.0f;
        if (in_regs) {
            if (mine) {
#pragma unroll
                for (int q = 0; q < RMAX; ++q) if (q * NW + mf < T) s += dbv[q];
            }
        } else {
            for (int idx = tid; idx < n_mels * tv; idx += THREADS) s += orow[(size_t)(idx / tv) * t_pad + idx % tv];
        }
        const double cnt = (double)n_mels * (in_regs ? T : tv);
        mean = (float)(block_sum(s, red, lane, wv) / cnt);
        float q2 = 0.0f;
        if (in_regs) {
            if (mine) {
#pragma unroll
                for (int q = 0; q < RMAX; ++q) if (q * NW + mf < T) { const float d = dbv[q] - mean; q2 += d * d; }
            }
        } else {
            for (int idx = tid; idx < n_mels * tv; idx += THREADS) { const float d = orow[(size_t)(idx / tv) * t_pad + idx % tv] - mean; q2 += d * d; }
        }
        const double m2 = block_sum(q2, red, lane, wv);
        denom = (cnt > 1.0 ? (float)sqrt(m2 / (cnt - 1.0)) : 0.0f) + NORM_EPS;
    }
    int tm0 = 0, tmw = 0, fm0 = 0, fmw = 0;
    if (time_mask) { tm0 = time_mask[2 * b]; tmw = time_mask[2 * b + 1]; }
    if (freq_mask) { fm0 = freq_mask[2 * b]; fmw = freq_mask[2 * b + 1]; }
    if (in_regs) {
        // every thread stores its own values: 16 lanes = 16 consecutive frames of one mel row (64-byte segments)
        if (mine) {
            const bool fmasked = md.x >= fm0 && md.x < fm0 + fmw;
            float* o = orow + (size_t)md.x * t_pad;
            float* dbo = drow ? drow + (size_t)md.x * t_pad : nullptr;
#pragma unroll
            for (int q = 0; q < RMAX; ++q) {
                const int t = q * NW + mf;
                if (t < t_pad) {
                    float v = 0.0f, d = 0.0f;
                    if (t < tv) {
                        d = dbv[q];
                        v = (d - mean) / denom;
                        if ((t >= tm0 && t < tm0 + tmw) || fmasked) v = 0.0f;
                    }
                    o[t] = v;
                    if (dbo) dbo[t] = d;
                }
            }
            for (int t = RMAX * NW + mf; t < t_pad; t += NW) {       // padding beyond the register tile
                o[t] = 0.0f;
                if (dbo) dbo[t] = 0.0f;
            }
        }
    } else {
        for (int idx = tid; idx < n_mels * t_pad; idx += THREADS) {
            const int mel = idx / t_pad, t = idx - mel * t_pad;
            float v = 0.0f, d = 0.0f;
            if (t < tv) {
                d = orow[idx];
                v = (d - mean) / denom;
                if ((t >= tm0 && t < tm0 + tmw) || (mel >= fm0 && mel < fm0 + fmw)) v = 0.0f;
            }
            orow[idx] = v;
            if (drow) drow[idx] = d;
        }
    }
}

// ---- gradient of the feature path with respect to the waveform (sir_features_bwd) ----------------------------------------
// feat_utt_bwd_kernel: the forward's geometry again -- one workgroup of 16 waves per utterance, rounds of 16 frames -- walked
// once, forward and backward of a frame in the same round, so nothing but db / dout is read and nothing but dwave written:
//   prologue: mean and sigma of the clip's dB tile (the forward's own two passes over db), then mean(g) and sum(g c) of the masked
//     dout; ordered wave sums, combined in double (block_sum).
//   round:  (1) wave w loads, windows and transforms frame 16 r + w as the forward does; the spectrum X stays in registers (8 bins
//     per lane + bin 512), the power row goes to P.                                                               barrier
//     (2) mel thread (frame, filter) recomputes M with the forward's own fmaf chain and writes dM = dD (10 / ln 10) / M (0 under
//     the 1e-10 clamp) into a [16][64] tile.                                                                      barrier
//     (3) wave w gathers dP of its bins (two taps each: MelTap), forms H = dP X, tangles it into the 512 complex points whose
//     transform is the frame's 1024 real outputs (the mirror of the untangle; the inverse transform is fft512 of the conjugate,
//     conjugated), windows them and leaves them in its own slab (4 KB of its 4.6 KB).                             barrier
//     (4) overlap-add: hop block q = second half of frame q + first half of frame q + 1; a round writes blocks 16 r - 1 .. 16 r + 14
//     (8 samples per thread, coalesced), the second half of the round's last frame is carried in LDS.              barrier
//   The reflect padding folds back in the same pass: frame 0's first half lands reversed on samples 1 .. 512, frame T - 1's part
//   beyond L on the tail -- both frames are in the slabs when those samples are written, except the one sample 512 (T - 2) - 1 of a
//   clip whose length is a multiple of the hop, which the same workgroup read-modify-writes at the end.
// No atomics, no workspace; every sum has a fixed order, so a row's bits depend on nothing but the row.
struct MelTap { int fa; float wa; int fb; float wb; };      // the (at most) two filters that cover an FFT bin, ascending; weight 0 = none
constexpr int DMS = 65;          // row stride of the dM tile: the 16 frames a filter's threads write fall on 16 banks
constexpr float DB_SCALE = 4.34294481903251827651f;       // 10 / ln 10

template <typename WT, bool AUG>
__global__ __launch_bounds__(THREADS) void feat_utt_bwd_kernel(
    const WT* __restrict__ wave, long long wave_stride, const int32_t* __restrict__ lengths, int max_len,
    const float* __restrict__ db, const float* __restrict__ dout, int t_pad, FeatTables tb, const MelTap* __restrict__ taps,
    AugArgs aug, const int32_t* __restrict__ time_mask, const int32_t* __restrict__ freq_mask,
    float* __restrict__ dwave, long long dwave_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cf32* xall = reinterpret_cast<cf32*>(smem);                        // [NW][XBUF] exchange slabs; after step 3: [NW][1024] frame gradients
    double* red = reinterpret_cast<double*>(xall + NW * XBUF);         // [NW] reduction scratch
    float* P = reinterpret_cast<float*>(red + NW);                     // [NW][PROW] power spectra of the round
    float* dmt = P + NW * PROW;                                        // [NW][DMS] dM of the round
    float* carry = dmt + NW * DMS;                                     // [512] second half of the previous round's last frame
    MelTap* tapl = reinterpret_cast<MelTap*>(carry + 512);             // [513 (+3)]
    float* melw = reinterpret_cast<float*>(tapl + 516);                // [mel_nnz]
    cf32* winl = reinterpret_cast<cf32*>(melw + ((tb.mel_nnz + 3) & ~3));       // [512] Hann window as sample pairs
    cf32* twul = winl + 512;                                           // [512] -i/2 * W1024^k
    cf32* tw2l = twul + 512;                                           // [8][TW2S]
    cf32* tw1l = tw2l + 8 * TW2S;                                      // [8][64] W512^(lane * k), row k (16 registers the spectrum needs here)

    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n_mels = tb.n_mels;
    int L = lengths[b];
    if (L > max_len) L = max_len;
    float* dw = dwave + (size_t)b * dwave_stride;
    const int T = (L > SIR_HOP) ? 1 + L / SIR_HOP : 0;                 // the host checked T <= t_pad
    if (T == 0) {                                                      // block-uniform: the forward gives a constant zero row
        for (int s = tid; s < max_len; s += THREADS) dw[s] = 0.0f;
        return;
    }
    const float* drow = db + (size_t)b * n_mels * t_pad;
    const float* grow = dout + (size_t)b * n_mels * t_pad;
    int tm0 = 0, tmw = 0, fm0 = 0, fmw = 0;
    if (time_mask) { tm0 = time_mask[2 * b]; tmw = time_mask[2 * b + 1]; }
    if (freq_mask) { fm0 = freq_mask[2 * b]; fmw = freq_mask[2 * b + 1]; }

    for (int i = tid; i < tb.mel_nnz; i += THREADS) melw[i] = tb.melw[i];
    if (tid < SIR_NFREQ) tapl[tid] = taps[tid];
    if (tid < 512) {
        winl[tid] = reinterpret_cast<const cf32*>(tb.window)[tid];
        twul[tid] = 0.5f * mul_mi(CF(tb.tw1024[tid]));
    }
    if (tid < 64) tw2l[(tid >> 3) * TW2S + (tid & 7)] = CF(tb.tw512[(8 * (tid >> 3) * (tid & 7)) & 511]);
    if (tid < 512) tw1l[tid] = CF(tb.tw512[((tid & 63) * (tid >> 6)) & 511]);

    // ---- statistics of the z-norm and of its gradient, over all n_mels * T positions ----
    const int n = n_mels * T;
    const double cnt = (double)n;
    float s_d = 0.0f, s_g = 0.0f;
    for (int idx = tid; idx < n; idx += THREADS) {
        const int f = idx / T, t = idx - f * T;
        s_d += drow[(size_t)f * t_pad + t];
        const bool masked = (t >= tm0 && t < tm0 + tmw) || (f >= fm0 && f < fm0 + fmw);
        s_g += masked ? 0.0f : grow[(size_t)f * t_pad + t];
    }
    const float mean = (float)(block_sum(s_d, red, lane, wv) / cnt);
    const float mean_g = (float)(block_sum(s_g, red, lane, wv) / cnt);
    float s_cc = 0.0f, s_gc = 0.0f;
    for (int idx = tid; idx < n; idx += THREADS) {
        const int f = idx / T, t = idx - f * T;
        const float c = drow[(size_t)f * t_pad + t] - mean;
        s_cc += c * c;
        const bool masked = (t >= tm0 && t < tm0 + tmw) || (f >= fm0 && f < fm0 + fmw);
        s_gc += masked ? 0.0f : grow[(size_t)f * t_pad + t] * c;
    }
    const double m2 = block_sum(s_cc, red, lane, wv);
    const double gc = block_sum(s_gc, red, lane, wv);
    const float sigma = (float)sqrt(m2 / (cnt - 1.0));
    const float den = sigma + NORM_EPS;
    const float inv_den = 1.0f / den;
    // dD = (g - mean g) / den - c * k2; a constant tile (sigma == 0) keeps the first term only
    const float k2 = sigma > 0.0f ? (float)(gc / ((double)den * (double)den * (double)sigma * (cnt - 1.0))) : 0.0f;

    const int mf = tid & 15;
    const int4 md = tb.mel_desc[tid >> 4];
    const bool fmasked = md.x >= fm0 && md.x < fm0 + fmw;

    const int m1p = lane & 7;
    const cf32* tw1 = tw1l + lane;
    const WT* x = wave + (size_t)b * wave_stride;
    int shift = 0;
    float sigma_n = 0.0f;
    if (AUG) {
        if (aug.shift) shift = aug.shift[b];
        if (aug.sigma) sigma_n = aug.sigma[b];
    }
    cf32* xb = xall + wv * XBUF;
    const int mirror = ((64 - lane) & 63) * 4;
    const unsigned a_win = lds_addr(winl + lane);
    const unsigned a_p2 = lds_addr(xb + (lane >> 3) * XS + m1p);
    unsigned a_p3[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a_p3[q] = lds_addr(xb + (lane & 7) * XS2 + ((lane >> 3) ^ q));
    const int nrounds = (T + NW - 1) / NW;
    const float* slabs = reinterpret_cast<const float*>(xall);         // frame gradient of wave w: slabs[w * 2 * XBUF + 0 .. 1023]
    constexpr int SLAB = 2 * XBUF;
    const float* last = slabs + ((T - 1) & (NW - 1)) * SLAB;           // frame T - 1 (valid in the last round and after it)
    const int last0 = (T - 1) * SIR_HOP - SIR_HOP;                     // its first padded sample

    cf32 nxt[8];
    if (wv < T) load_frame<WT, AUG>(x, L, wv, lane, shift, sigma_n, aug.seed, b, nxt);
    __syncthreads();                                                   // tables are staged

    for (int r = 0; r < nrounds; ++r) {
        const int t = r * NW + wv;
        cf32 X[8];
        float x512 = 0.0f;
        if (t < T) {                                                   // (1) wave-uniform: the forward's transform of frame t
            cf32 v[8];
            lds_read8<64 * 8>(a_win, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = nxt[j] * v[j];
            if (t + NW < T) load_frame<WT, AUG>(x, L, t + NW, lane, shift, sigma_n, aug.seed, b, nxt);
            fft512(v, tw1, tw2l + TW2S * m1p, xb, lane, a_p2, a_p3);
            float* prow = P + wv * PROW;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const cf32 z = v[j];
                cf32 zc;
                zc.x = __int_as_float(__builtin_amdgcn_ds_bpermute(mirror, __float_as_int(v[7 - j].x)));
                zc.y = __int_as_float(__builtin_amdgcn_ds_bpermute(mirror, __float_as_int(v[7 - j].y)));
                if (lane == 0) zc = v[(8 - j) & 7];
                zc.y = -zc.y;
                const cf32 xk = 0.5f * (z + zc) + cmul(z - zc, twul[lane + 64 * j]);
                const cf32 sq = xk * xk;
                prow[lane + 64 * j] = sq.x + sq.y;
                X[j] = xk;
            }
            x512 = v[0].x - v[0].y;                                    // X[512] (lane 0's is the one used)
            if (lane == 0) prow[512] = x512 * x512;
        }
        __syncthreads();
        {   // (2) dM[frame mf][filter md.x]
            const int tm = r * NW + mf;
            float dm = 0.0f;
            if (md.x >= 0 && tm < T) {
                const float* pr = P + mf * PROW + md.y;
                const float* wr = melw + md.w;
                float acc = 0.0f;
                for (int i = 0; i < md.z; ++i) acc = fmaf(wr[i], pr[i], acc);
                if (acc > AMIN) {                                      // the forward's clamp: at or below it the output is the constant -100
                    const size_t o = (size_t)md.x * t_pad + tm;
                    const bool masked = (tm >= tm0 && tm < tm0 + tmw) || fmasked;
                    const float g = masked ? 0.0f : grow[o];
                    const float c = drow[o] - mean;
                    dm = ((g - mean_g) * inv_den - c * k2) * DB_SCALE / acc;
                }
            }
            if (md.x >= 0) dmt[mf * DMS + md.x] = dm;
        }
        __syncthreads();
        if (t < T) {                                                   // (3) dP -> H -> tangle -> inverse transform -> window
            const float* dmr = dmt + wv * DMS;
            cf32 h[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const MelTap tp = tapl[lane + 64 * j];
                const float dp = fmaf(tp.wb, dmr[tp.fb], tp.wa * dmr[tp.fa]);
                h[j] = dp * X[j];
            }
            const MelTap tp = tapl[512];
            const float h512 = fmaf(tp.wb, dmr[tp.fb], tp.wa * dmr[tp.fa]) * x512;
            if (lane == 0) h[0] = cf32{2.0f * h[0].x, 0.0f};           // bins 0 and 512 count once, the interior ones twice
            cf32 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                // G[k] = (H[k] + conj H[512-k]) + i e^(+2 pi i k / 1024) (H[k] - conj H[512-k]); v = conj G
                cf32 hp;
                hp.x = __int_as_float(__builtin_amdgcn_ds_bpermute(mirror, __float_as_int(h[7 - j].x)));
                hp.y = __int_as_float(__builtin_amdgcn_ds_bpermute(mirror, __float_as_int(h[7 - j].y)));
                if (lane == 0) hp = (j == 0) ? cf32{2.0f * h512, 0.0f} : h[(8 - j) & 7];
                const cf32 hc = cf32{h[j].x, -h[j].y};
                v[j] = (hc + hp) + 2.0f * cmul(hc - hp, twul[lane + 64 * j]);
            }
            fft512(v, tw1, tw2l + TW2S * m1p, xb, lane, a_p2, a_p3);
            cf32 w[8];
            lds_read8<64 * 8>(a_win, w);
            wave_fence();
#pragma unroll
            for (int j = 0; j < 8; ++j) xb[lane + 64 * j] = cf32{v[j].x, -v[j].y} * w[j];   // samples 2 m, 2 m + 1 of the frame, m = lane + 64 j
            wave_fence();
        }
        __syncthreads();
        // (4) overlap-add of hop blocks 16 r - 1 .. 16 r + 14 (those up to T - 2: block T - 1 follows the loop)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int idx = tid + THREADS * k;
            const int q = r * NW - 1 + (idx >> 9), o = idx & 511;
            if (q >= 0 && q <= T - 2) {
                const int i = q * SIR_HOP + o;
                float val = (q == r * NW - 1) ? carry[o] : slabs[(q & (NW - 1)) * SLAB + 512 + o];
                val += slabs[((q + 1) & (NW - 1)) * SLAB + o];
                if (i >= 1 && i <= SIR_HOP) val += slabs[SIR_HOP - i];                  // reflected head: frame 0 (round 0)
                const int ip = 2 * L - 2 - i;                                            // reflected tail: frame T - 1
                if (q == T - 2 && ip >= L && ip < T * SIR_HOP) val += last[ip - last0];
                const int s = i - shift;
                if (s >= 0 && s < L) dw[s] = val;
            }
        }
        if (tid < 512) carry[tid] = slabs[(NW - 1) * SLAB + 512 + tid];               // (read above by this thread only)
        __syncthreads();                                               // the slabs are free again
    }
    // block T - 1: the second half of the last frame, as far as the clip goes
    if (tid < 512) {
        const int i = (T - 1) * SIR_HOP + tid;
        if (i < L) {
            float val = last[512 + tid];
            if (i <= SIR_HOP) val += slabs[SIR_HOP - i];              // T == 2: sample 512 under frame 0's first sample
            const int ip = 2 * L - 2 - i;
            if (ip >= L && ip < T * SIR_HOP) val += last[ip - last0];
            const int s = i - shift;
            if (s >= 0 && s < L) dw[s] = val;
        }
    }
    // samples that no padded position feeds: shifted out of the clip, or beyond it
    for (int s = tid; s < max_len; s += THREADS)
        if (s >= L || s + shift < 0 || s + shift >= L) dw[s] = 0.0f;
    // a length that is a multiple of the hop: the last padded sample folds onto 512 (T - 2) - 1, a block written before frame
    // T - 1 was there when that frame opens a round -- added here in every case (same workgroup, behind the round's barrier)
    if (tid == 0 && L == (T - 1) * SIR_HOP) {
        const int s = (T - 2) * SIR_HOP - 1 - shift;
        if (s >= 0 && s < L) dw[s] += last[1023];
    }
}

// ---- general forward path: every front-end but n_fft 1024 / hop 512 / win_length 1024 ------------------------------------------
// n_fft in {256, 512, 1024}, any hop in [n_fft/16, n_fft], a window of win_length <= n_fft samples centred in the frame.  A clip
// at hop 64 has 1251 frames, so nothing is kept in registers and the statistics travel through a workspace slab: a launch PAIR.
//   feat_gen_frames_kernel: grid (utterance, tile of GEN_FT frames), 16 waves, one wave per frame, rounds of 16 frames as in
//     feat_utt_kernel.  The n_fft/2 = 64 R1 packed points (R1 = 2, 4, 8 per lane) take one radix-R1 pass in registers and the two
//     radix-8 passes of the 64-point transforms that remain (8 lanes each: 8 R1 lanes work, the rest idle), through the wave's own
//     slab with feat_utt_kernel's two exchange layouts; the result is left in natural order in the slab, untangled from there
//     (Z[k] and Z[N - k] are two LDS reads: with R1 < 8 the partner is not one lane's register) and squared into row w of P.
//     After the round's barrier the 1024 threads take the 16 x 64 (frame, filter) dot products over the compact filterbank -- a
//     filter without taps (n_fft 256 has one) sums nothing and is exactly -100 dB -- and write dB to slab[b][filter][frame],
//     ALL frames of the clip, also those beyond t_pad.
//   feat_gen_norm_kernel: one workgroup per utterance reads its slab rows twice (mean, then centred squares; per-thread sums in
//     double, lanes then waves combined in a fixed order, no atomics), and stores (x - mean) / (std + 1e-5), the SpecAugment
//     bands, the dB copy and the zero padding.  Row b depends on row b alone and its bits do not change from run to run.
// Samples are loaded per frame: a frame start on a sample-pair boundary takes the two-samples-per-word loads, any other one (odd
// hops) element loads; frames that touch the reflect padding, and every frame under time shift / noise, go through fetch().
constexpr int GEN_FT = 64;       // frames per workgroup of feat_gen_frames_kernel

struct GenTables {
    const float2* twn;           // W_N^k, N = n_fft / 2, k < N
    const float2* tw2n;          // W_2N^k, k < N
    const float* window;         // [n_fft], the window centred between zeros
    const float* melw;
    const int4* mel_desc;
    int mel_nnz;
    int n_mels;
    int hop;
};

// forward R-point DFT of v[0 .. R), natural order in and out
template <int R> __device__ __forceinline__ void dft_small(cf32 (&v)[8]);
template <> __device__ __forceinline__ void dft_small<8>(cf32 (&v)[8]) { dft8(v); }
template <> __device__ __forceinline__ void dft_small<4>(cf32 (&v)[8]) {
    const cf32 a0 = v[0] + v[2], a1 = v[0] - v[2], a2 = v[1] + v[3], a3 = mul_mi(v[1] - v[3]);
    v[0] = a0 + a2; v[2] = a0 - a2; v[1] = a1 + a3; v[3] = a1 - a3;
}
template <> __device__ __forceinline__ void dft_small<2>(cf32 (&v)[8]) {
    const cf32 a = v[0] + v[1], d = v[0] - v[1];
    v[0] = a; v[1] = d;
}

// the 2 R1 samples of one lane for the frame that starts at clip sample `base` (pairs (i0, i0 + 1), i0 = base + 2 (lane + 64 j))
template <typename T, bool AUG, int R1>
__device__ __forceinline__ void load_frame_gen(const T* __restrict__ x, int L, int base, int lane, int shift, float sigma,
                                               unsigned long long seed, int b, cf32 (&s)[8]) {
    constexpr int NFFT = 128 * R1;
    const bool interior = base >= 0 && base + NFFT <= L;               // wave-uniform: no reflection in this frame
    if (interior && !AUG) {
        const T* q = x + base;
        if ((reinterpret_cast<uintptr_t>(q) & (2 * sizeof(T) - 1)) == 0) {        // the frame starts on a sample-pair boundary
            if (sizeof(T) == 4) {
                const cf32* p = reinterpret_cast<const cf32*>(q) + lane;
#pragma unroll
                for (int j = 0; j < R1; ++j) s[j] = p[64 * j];
            } else {
                const unsigned* p = reinterpret_cast<const unsigned*>(q) + lane;
#pragma unroll
                for (int j = 0; j < R1; ++j) {
                    const unsigned w = p[64 * j];
                    s[j] = cf32{(float)(short)(w & 0xFFFFu), (float)(short)(w >> 16)} * (1.0f / 32768.0f);
                }
            }
        } else {                                                        // odd hop / odd row offset: element loads
#pragma unroll
            for (int j = 0; j < R1; ++j) {
                const T* e = q + 2 * (lane + 64 * j);
                s[j] = cf32{to_f32<T>(e[0]), to_f32<T>(e[1])};
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < R1; ++j) {                  // reflect padding and / or augmentation: a pure function of the sample index
        const int i0 = base + 2 * (lane + 64 * j);
        s[j].x = fetch<T, AUG>(x, L, i0, shift, sigma, seed, b);
        s[j].y = fetch<T, AUG>(x, L, i0 + 1, shift, sigma, seed, b);
    }
}

template <typename WT, bool AUG, int R1>
__global__ __launch_bounds__(THREADS) void feat_gen_frames_kernel(
    const WT* __restrict__ wave, long long wave_stride, const int32_t* __restrict__ lengths, int max_len,
    float* __restrict__ slab, int slab_t, GenTables tb, AugArgs aug) {
    constexpr int N = 64 * R1;                      // complex points of the packed transform
    constexpr int XB = R1 * XS;                     // complex slots of a wave's slab (>= N, and >= the second exchange's R1 * XS2)
    constexpr int PR = N + 2;                       // words per power-spectrum row (= 2 mod 64: 16 frames on 16 banks)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cf32* xall = reinterpret_cast<cf32*>(smem);                        // [NW][XB]
    float* Pbuf = reinterpret_cast<float*>(xall + NW * XB);            // [2][NW][PR], by round parity
    float* melw = Pbuf + 2 * NW * PR;                                  // [mel_nnz]
    cf32* winl = reinterpret_cast<cf32*>(melw + ((tb.mel_nnz + 3) & ~3));       // [N] window as sample pairs
    cf32* twnl = winl + N;                                             // [N] W_N^k
    cf32* twul = twnl + N;                                             // [N] -i/2 * W_2N^k, the untangle twiddles

    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int L = lengths[b];
    if (L > max_len) L = max_len;
    const int hop = tb.hop;
    const int T = (L > N) ? 1 + L / hop : 0;                           // L <= n_fft/2: the reference fails (reflect pad) -> zero row
    const int t0 = blockIdx.y * GEN_FT;
    if (t0 >= T) return;                                               // block-uniform
    const int t1 = (T < t0 + GEN_FT) ? T : t0 + GEN_FT;

    for (int i = tid; i < tb.mel_nnz; i += THREADS) melw[i] = tb.melw[i];
    if (tid < N) {
        winl[tid] = reinterpret_cast<const cf32*>(tb.window)[tid];
        twnl[tid] = CF(tb.twn[tid]);
        twul[tid] = 0.5f * mul_mi(CF(tb.tw2n[tid]));
    }
    cf32 tw1[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) tw1[k] = (k < R1) ? CF(tb.twn[lane * k]) : cf32{1.0f, 0.0f};       // W_N^(n1 k2); lane * k < N
    const WT* x = wave + (size_t)b * wave_stride;
    int shift = 0;
    float sigma = 0.0f;
    if (AUG) {
        if (aug.shift) shift = aug.shift[b];
        if (aug.sigma) sigma = aug.sigma[b];
    }
    cf32* xb = xall + wv * XB;
    const int mf = tid & 15;
    const int4 md = tb.mel_desc[tid >> 4];                             // {filter, first bin, taps, offset}
    float* srow = slab + (size_t)b * tb.n_mels * slab_t;
    __syncthreads();                                                   // tables are staged

    const int nrounds = (t1 - t0 + NW - 1) / NW;
    for (int r = 0; r < nrounds; ++r) {
        const int t = t0 + r * NW + wv;
        float* P = Pbuf + (r & 1) * (NW * PR);
        if (t < t1) {                                                  // wave-uniform
            cf32 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = cf32{0.0f, 0.0f};
            load_frame_gen<WT, AUG, R1>(x, L, t * hop - N, lane, shift, sigma, aug.seed, b, v);
#pragma unroll
            for (int j = 0; j < R1; ++j) v[j] = v[j] * winl[lane + 64 * j];
            // pass 1: point n = n1 + 64 n2 (n1 = lane): DFT over n2 -> k2, twiddle W_N^(n1 k2)
            dft_small<R1>(v);
#pragma unroll
            for (int k = 1; k < R1; ++k) v[k] = cmul(v[k], tw1[k]);
            wave_fence();
#pragma unroll
            for (int k = 0; k < R1; ++k) xb[k * XS + lane] = v[k];
            wave_fence();
            {   // pass 2: lane = (k2, m1), n1 = m1 + 8 m2: DFT over m2 -> j2, twiddle W64^(m1 j2) = W_N^(R1 m1 j2)
                const int k2 = lane >> 3, m1p = lane & 7;
                const bool act = k2 < R1;
                if (act) {
#pragma unroll
                    for (int m = 0; m < 8; ++m) v[m] = xb[k2 * XS + m1p + 8 * m];
                    dft8(v);
#pragma unroll
                    for (int k = 1; k < 8; ++k) v[k] = cmul(v[k], twnl[R1 * m1p * k]);
                }
                wave_fence();
                if (act) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) xb[ex2_index(k2, j, m1p)] = v[j];
                }
                wave_fence();
            }
            {   // pass 3: lane = (j2, k2): DFT over m1 -> j1; bin k = k2 + R1 (j2 + 8 j1), stored in natural order
                const int k2 = lane & 7, j2 = lane >> 3;
                const bool act = k2 < R1;
                if (act) {
#pragma unroll
                    for (int m = 0; m < 8; ++m) v[m] = xb[ex2_index(k2, j2, m)];
                    dft8(v);
                }
                wave_fence();
                if (act) {
#pragma unroll
                    for (int j1 = 0; j1 < 8; ++j1) xb[k2 + R1 * (j2 + 8 * j1)] = v[j1];
                }
                wave_fence();
            }
            // untangle the packed real transform: X[k] = (z + conj zp)/2 + (-i/2 W_2N^k)(z - conj zp), zp = Z[N - k] (Z[N] = Z[0])
            float* prow = P + wv * PR;
#pragma unroll
            for (int j = 0; j < R1; ++j) {
                const int k = lane + 64 * j;
                const cf32 z = xb[k];
                cf32 zc = xb[(N - k) & (N - 1)];
                zc.y = -zc.y;
                const cf32 xk = 0.5f * (z + zc) + cmul(z - zc, twul[k]);
                const cf32 sq = xk * xk;
                prow[k] = sq.x + sq.y;
            }
            if (lane == 0) { const cf32 z0 = xb[0]; const float n = z0.x - z0.y; prow[N] = n * n; }      // X[N] = Re Z0 - Im Z0
        }
        __syncthreads();                                // all spectra of this round are in P (the other parity is free again)
        const int tm = t0 + r * NW + mf;
        if (md.x >= 0 && tm < t1) {
            const float* pr = P + mf * PR + md.y;
            const float* wr = melw + md.w;
            float acc = 0.0f;
            for (int i = 0; i < md.z; ++i) acc = fmaf(wr[i], pr[i], acc);
            srow[(size_t)md.x * slab_t + tm] = (acc <= AMIN) ? -100.0f : 10.0f * log10f(acc);
        }
    }
}

// one double per thread summed over the workgroup in a fixed order (lanes by xor-shuffle, then the 16 waves in index order)
__device__ __forceinline__ double block_sum_f64(double v, double* red, int lane, int wv) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if (lane == 0) red[wv] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) s += red[i];
    return s;
}

__global__ __launch_bounds__(THREADS) void feat_gen_norm_kernel(
    const float* __restrict__ slab, int slab_t, const int32_t* __restrict__ lengths, int max_len, int half_fft, int hop, int n_mels,
    float* __restrict__ out, float* __restrict__ db_out, int t_pad, const int32_t* __restrict__ time_mask,
    const int32_t* __restrict__ freq_mask) {
    __shared__ double red[NW];
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int L = lengths[b];
    if (L > max_len) L = max_len;
    const int T = (L > half_fft) ? 1 + L / hop : 0;
    const int tv = T < t_pad ? T : t_pad;
    const float* srow = slab + (size_t)b * n_mels * slab_t;
    float* orow = out + (size_t)b * n_mels * t_pad;
    float* drow = db_out ? db_out + (size_t)b * n_mels * t_pad : nullptr;
    // statistics over ALL T frames of the clip (the reference normalises before any trim); wave w walks mel rows w, w + 16, ...
    float mean = 0.0f, denom = 1.0f;
    if (T > 0) {
        double s = 0.0;
        for (int f = wv; f < n_mels; f += NW)
            for (int t = lane; t < T; t += 64) s += (double)srow[(size_t)f * slab_t + t];
        const double cnt = (double)n_mels * T;
        mean = (float)(block_sum_f64(s, red, lane, wv) / cnt);
        double q2 = 0.0;
        for (int f = wv; f < n_mels; f += NW)
            for (int t = lane; t < T; t += 64) { const float d = srow[(size_t)f * slab_t + t] - mean; q2 += (double)(d * d); }
        const double m2 = block_sum_f64(q2, red, lane, wv);
        denom = (cnt > 1.0 ? (float)sqrt(m2 / (cnt - 1.0)) : 0.0f) + NORM_EPS;
    }
    int tm0 = 0, tmw = 0, fm0 = 0, fmw = 0;
    if (time_mask) { tm0 = time_mask[2 * b]; tmw = time_mask[2 * b + 1]; }
    if (freq_mask) { fm0 = freq_mask[2 * b]; fmw = freq_mask[2 * b + 1]; }
    for (int f = wv; f < n_mels; f += NW) {
        const bool fmasked = f >= fm0 && f < fm0 + fmw;
        for (int t = lane; t < t_pad; t += 64) {
            float v = 0.0f, d = 0.0f;
            if (t < tv) {
                d = srow[(size_t)f * slab_t + t];
                v = (d - mean) / denom;
                if ((t >= tm0 && t < tm0 + tmw) || fmasked) v = 0.0f;
            }
            orow[(size_t)f * t_pad + t] = v;
            if (drow) drow[(size_t)f * t_pad + t] = d;
        }
    }
}

size_t gen_slab_bytes(const sir_handle* h, int batch, int max_len) {
    return sir_align_up((size_t)batch * h->cfg.n_mels * (size_t)(1 + max_len / h->cfg.hop_length) * sizeof(float), 256);
}

template <int R1>
int launch_gen(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride, const int32_t* lengths, int batch,
               int max_len, float* out, int t_pad, float* db_out, void* workspace, const sir_augment* aug, hipStream_t stream) {
    constexpr int N = 64 * R1;
    const int hop = h->cfg.hop_length, slab_t = 1 + max_len / hop;
    const int tiles = (slab_t + GEN_FT - 1) / GEN_FT;
    const size_t lds = sir_features_gen_lds_bytes(h->cfg.n_fft, h->mel_nnz);       // (sir_create_ex checked it against the LDS)
    if (tiles > 65535) {
        sir_set_error("sir_features_fwd: %d frames per clip are beyond the general feature path (<= %d frames)", slab_t,
                      65535 * GEN_FT);
        return SIR_EUNSUPPORTED;
    }
    GenTables tb{h->gen_twn, h->gen_tw2n, h->window, h->melw, h->mel_desc, h->mel_nnz, h->cfg.n_mels, hop};
    AugArgs ag{nullptr, nullptr, 0ull};
    bool wave_aug = false;
    const int32_t *tmask = nullptr, *fmask = nullptr;
    if (aug) {
        ag.shift = aug->shift; ag.sigma = aug->noise_sigma; ag.seed = aug->noise_seed;
        wave_aug = aug->shift || aug->noise_sigma;
        tmask = aug->time_mask; fmask = aug->freq_mask;
    }
    float* slab = reinterpret_cast<float*>(workspace);
    dim3 grid(batch, tiles), block(THREADS);
#define SIR_LAUNCH_GEN(TY, AUGF)                                                                                  \
    SIR_TRY(sir_lds_opt_in(h, (const void*)feat_gen_frames_kernel<TY, AUGF, R1>, (int)lds));                     \
    hipLaunchKernelGGL((feat_gen_frames_kernel<TY, AUGF, R1>), grid, block, lds, stream, (const TY*)wave,        \
                       (long long)wave_stride, lengths, max_len, slab, slab_t, tb, ag)
    SirProfScope prof(h, SIR_K_FEAT_FRAMES, stream);                   // the pair is timed under the one id
    if (wave_dtype == SIR_WAVE_F32) { if (wave_aug) { SIR_LAUNCH_GEN(float, true); } else { SIR_LAUNCH_GEN(float, false); } }
    else { if (wave_aug) { SIR_LAUNCH_GEN(short, true); } else { SIR_LAUNCH_GEN(short, false); } }
#undef SIR_LAUNCH_GEN
    hipLaunchKernelGGL(feat_gen_norm_kernel, dim3(batch), block, 0, stream, slab, slab_t, lengths, max_len, N, hop,
                       h->cfg.n_mels, out, db_out, t_pad, tmask, fmask);
    return SIR_OK;
}

}  // namespace

// dynamic LDS of feat_gen_frames_kernel: exchange slabs, two power-spectrum buffers, filter weights, window + two twiddle tables
size_t sir_features_gen_lds_bytes(int n_fft, int mel_nnz) {
    const int n = n_fft / 2, r1 = n / 64;
    return (size_t)NW * r1 * XS * sizeof(float2) + (size_t)2 * NW * (n + 2) * sizeof(float) +
           (size_t)((mel_nnz + 3) & ~3) * sizeof(float) + (size_t)3 * n * sizeof(float2);
}

extern "C" size_t sir_features_workspace_bytes(const sir_handle* h, int batch, int max_len) {
    if (batch <= 0 || max_len <= 0) return 0;
    if (h && h->general) return gen_slab_bytes(h, batch, max_len);     // the launch pair's dB slab: every frame of every clip
    return 256;          // the fused kernel keeps its statistics on chip; a token size keeps the (workspace, bytes) contract
}

int sir_features_launch(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride,
                        const int32_t* lengths, int batch, int max_len, float* out, int t_pad,
                        float* db_out, void* workspace, size_t workspace_bytes, const sir_augment* aug,
                        hipStream_t stream) {
    if (!h || !wave || !lengths || !out || !workspace) { sir_set_error("sir_features_fwd: NULL argument"); return SIR_EINVAL; }
    if (batch <= 0 || max_len <= 0 || t_pad <= 0 || wave_stride < max_len) {
        sir_set_error("sir_features_fwd: bad shape batch=%d max_len=%d t_pad=%d stride=%lld", batch, max_len, t_pad,
                      (long long)wave_stride);
        return SIR_EINVAL;
    }
    if (wave_dtype != SIR_WAVE_F32 && wave_dtype != SIR_WAVE_I16) { sir_set_error("sir_features_fwd: wave_dtype %d", wave_dtype); return SIR_EINVAL; }
    if (workspace_bytes < sir_features_workspace_bytes(h, batch, max_len)) { sir_set_error("sir_features_fwd: workspace too small"); return SIR_ENOMEM; }
    const size_t esz = wave_dtype == SIR_WAVE_F32 ? 4 : 2;
    if (((uintptr_t)wave % esz) != 0) { sir_set_error("sir_features_fwd: waveform pointer is not aligned to its sample type"); return SIR_EINVAL; }
    if (h->general) {
        if (((uintptr_t)workspace % 16) != 0) { sir_set_error("sir_features_fwd: the workspace is not 16-byte aligned"); return SIR_EINVAL; }
        int rc;
        switch (h->cfg.n_fft) {
            case 256: rc = launch_gen<2>(h, wave, wave_dtype, wave_stride, lengths, batch, max_len, out, t_pad, db_out, workspace, aug, stream); break;
            case 512: rc = launch_gen<4>(h, wave, wave_dtype, wave_stride, lengths, batch, max_len, out, t_pad, db_out, workspace, aug, stream); break;
            default:  rc = launch_gen<8>(h, wave, wave_dtype, wave_stride, lengths, batch, max_len, out, t_pad, db_out, workspace, aug, stream); break;
        }
        SIR_TRY(rc);
        SIR_HIP_TRY(hipGetLastError());
        return SIR_OK;
    }
    const int max_t = 1 + max_len / SIR_HOP;
    if (max_t > TILE_T && max_t > t_pad) {
        // a clip longer than the LDS tile parks its dB values in its output rows; the statistics of the reference are
        // over ALL frames (precompute_features.py:73 normalises before any trim), so every frame needs a slot there
        sir_set_error("sir_features_fwd: clips of up to %d frames need t_pad >= %d (or max_len <= %d samples)", max_t, max_t,
                      TILE_T * SIR_HOP + SIR_HOP - 1);
        return SIR_EUNSUPPORTED;
    }
    FeatTables tb{h->tw512, h->tw1024, h->window, h->melw, h->mel_desc, h->mel_nnz, h->cfg.n_mels};
    AugArgs ag{nullptr, nullptr, 0ull};
    bool wave_aug = false;
    const int32_t *tmask = nullptr, *fmask = nullptr;
    if (aug) {
        ag.shift = aug->shift; ag.sigma = aug->noise_sigma; ag.seed = aug->noise_seed;
        wave_aug = aug->shift || aug->noise_sigma;
        tmask = aug->time_mask; fmask = aug->freq_mask;
    }
    const size_t lds = (size_t)NW * XBUF * sizeof(float2) + NW * sizeof(double) + (size_t)2 * NW * PROW * sizeof(float) +
                       (size_t)((h->mel_nnz + 3) & ~3) * sizeof(float) + (1024 + 8 * TW2S) * sizeof(float2);
    dim3 grid(batch), block(THREADS);
    // (> 64 KB of dynamic LDS needs the opt-in)
#define SIR_LAUNCH_FEAT(TY, AUGF)                                                                            \
    SIR_TRY(sir_lds_opt_in(h, (const void*)feat_utt_kernel<TY, AUGF>, (int)lds));                           \
    hipLaunchKernelGGL((feat_utt_kernel<TY, AUGF>), grid, block, lds, stream, (const TY*)wave,              \
                       (long long)wave_stride, lengths, max_len, out, db_out, t_pad, tb, ag, tmask, fmask)
    {
    SirProfScope prof(h, SIR_K_FEAT_FRAMES, stream);
    if (wave_dtype == SIR_WAVE_F32) { if (wave_aug) { SIR_LAUNCH_FEAT(float, true); } else { SIR_LAUNCH_FEAT(float, false); } }
    else { if (wave_aug) { SIR_LAUNCH_FEAT(short, true); } else { SIR_LAUNCH_FEAT(short, false); } }
    }
#undef SIR_LAUNCH_FEAT
    SIR_HIP_TRY(hipGetLastError());
    return SIR_OK;
}

int sir_features_bwd_launch(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride, const int32_t* lengths,
                            int batch, int max_len, const float* db, const float* dout, int t_pad, const sir_augment* aug,
                            float* dwave, int64_t dwave_stride, hipStream_t stream) {
    if (!h || !wave || !lengths || !db || !dout || !dwave) { sir_set_error("sir_features_bwd: NULL argument"); return SIR_EINVAL; }
    if (batch <= 0 || max_len <= 0 || t_pad <= 0 || wave_stride < max_len || dwave_stride < max_len) {
        sir_set_error("sir_features_bwd: bad shape batch=%d max_len=%d t_pad=%d wave_stride=%lld dwave_stride=%lld", batch, max_len,
                      t_pad, (long long)wave_stride, (long long)dwave_stride);
        return SIR_EINVAL;
    }
    if (wave_dtype != SIR_WAVE_F32 && wave_dtype != SIR_WAVE_I16) { sir_set_error("sir_features_bwd: wave_dtype %d", wave_dtype); return SIR_EINVAL; }
    const size_t esz = wave_dtype == SIR_WAVE_F32 ? 4 : 2;
    if (((uintptr_t)wave % esz) != 0 || ((uintptr_t)db % 4) != 0 || ((uintptr_t)dout % 4) != 0 || ((uintptr_t)dwave % 4) != 0) {
        sir_set_error("sir_features_bwd: a pointer is not aligned to its element type");
        return SIR_EINVAL;
    }
    const int max_t = 1 + max_len / SIR_HOP;
    if (max_t > t_pad) {
        // the statistics run over ALL frames of a clip, and db holds only t_pad of them
        sir_set_error("sir_features_bwd: clips of up to %d frames need t_pad >= %d (got %d)", max_t, max_t, t_pad);
        return SIR_EUNSUPPORTED;
    }
    if (h->mel_max_cover > 2) {
        sir_set_error("sir_features_bwd: an FFT bin lies in %d filters of the handle's filterbank; only banks of overlapping "
                      "neighbours (<= 2 per bin, as HTK triangles) are built", h->mel_max_cover);
        return SIR_EUNSUPPORTED;
    }
    FeatTables tb{h->tw512, h->tw1024, h->window, h->melw, h->mel_desc, h->mel_nnz, h->cfg.n_mels};
    AugArgs ag{nullptr, nullptr, 0ull};
    bool wave_aug = false;
    const int32_t *tmask = nullptr, *fmask = nullptr;
    if (aug) {
        ag.shift = aug->shift; ag.sigma = aug->noise_sigma; ag.seed = aug->noise_seed;
        wave_aug = aug->shift || aug->noise_sigma;
        tmask = aug->time_mask; fmask = aug->freq_mask;
    }
    const MelTap* taps = reinterpret_cast<const MelTap*>(h->mel_taps);
    const size_t lds = (size_t)NW * XBUF * sizeof(float2) + NW * sizeof(double) + (size_t)NW * PROW * sizeof(float) +
                       (size_t)NW * DMS * sizeof(float) + 512 * sizeof(float) + 516 * sizeof(MelTap) +
                       (size_t)((h->mel_nnz + 3) & ~3) * sizeof(float) + (1024 + 8 * TW2S + 512) * sizeof(float2);
    dim3 grid(batch), block(THREADS);
#define SIR_LAUNCH_FEAT_BWD(TY, AUGF)                                                                            \
    SIR_TRY(sir_lds_opt_in(h, (const void*)feat_utt_bwd_kernel<TY, AUGF>, (int)lds));                           \
    hipLaunchKernelGGL((feat_utt_bwd_kernel<TY, AUGF>), grid, block, lds, stream, (const TY*)wave,              \
                       (long long)wave_stride, lengths, max_len, db, dout, t_pad, tb, taps, ag, tmask, fmask,   \
                       dwave, (long long)dwave_stride)
    // (no SirProfScope: the profile id tables are closed; devtools/feat_only.py --backward times this launch with events)
    if (wave_dtype == SIR_WAVE_F32) { if (wave_aug) { SIR_LAUNCH_FEAT_BWD(float, true); } else { SIR_LAUNCH_FEAT_BWD(float, false); } }
    else { if (wave_aug) { SIR_LAUNCH_FEAT_BWD(short, true); } else { SIR_LAUNCH_FEAT_BWD(short, false); } }
#undef SIR_LAUNCH_FEAT_BWD
    SIR_HIP_TRY(hipGetLastError());
    return SIR_OK;
}
