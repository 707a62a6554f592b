// What the feature path's three stages share: features_fwd.hip (feat_utt_kernel, n_fft 1024 / hop 512), features_bwd.hip
// (feat_utt_bwd_kernel, its gradient) and features_gen.hip (the general launch pair).  Constants, the kernels' argument structs, the
// sample loads with their augmentation, the in-wave transform over wave_fft.h, the workgroup sum, and the host's augment unpacking
// and float | short x AUG dispatch.  LDS layouts: feat_lds.h.  The steps the backward repeats after the forward (table staging,
// untangle, mel fmaf chain) stay spelt out in each kernel, each naming its twin: as shared inline functions they compile to other
// instruction schedules, and these kernels have no register to spare.
#pragma once
#include <stdint.h>
#include <type_traits>
#include "sir_internal.h"
#include "wave_fft.h"
#include "wave_sample.h"
#include "feat_lds.h"

namespace {

constexpr int THREADS = NW * 64;
static_assert(XBUF == 8 * XS, "feat_lds.h: a wave's slab holds the 8 rows of the first exchange");
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

// 512-point complex DFT inside one wave: on entry lane holds points lane + 64 j, on return bins lane + 64 j (j = register).
// Three radix-8 passes with two exchanges through the wave's own slab xb; tw1col[64 k] = W512^(lane * k) in LDS, tw2row = row lane & 7 of the pass-2
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

// workgroup sum of one float or double per thread in a fixed order: lanes by xor-shuffle in the thread's own type, then the 16
// wave sums in index order in double; every thread gets the result
template <typename T>
__device__ __forceinline__ double block_sum(T v, double* red, int lane, int wv) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                 // red is reused across calls
    if (lane == 0) red[wv] = (double)v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) s += red[i];
    return s;
}

// ---- host side: what the three launch sites share ----------------------------------------------------------------------------
struct AugHost {                 // a sir_augment (or none) as the kernels take it
    AugArgs ag{nullptr, nullptr, 0ull};
    bool wave_aug = false;       // time shift and / or noise: the AUG instantiations
    const int32_t *tmask = nullptr, *fmask = nullptr;
    explicit AugHost(const sir_augment* aug) {
        if (!aug) return;
        ag.shift = aug->shift; ag.sigma = aug->noise_sigma; ag.seed = aug->noise_seed;
        wave_aug = aug->shift || aug->noise_sigma;
        tmask = aug->time_mask; fmask = aug->freq_mask;
    }
};

// launch(sample type, std::true_type | std::false_type AUG) for a waveform of `wave_dtype` (checked by the caller): the float | short x AUG instantiation to run
template <typename F>
int dispatch_wave(int wave_dtype, bool wave_aug, F&& launch) {
    if (wave_dtype == SIR_WAVE_F32) return wave_aug ? launch(float(), std::true_type()) : launch(float(), std::false_type());
    return wave_aug ? launch(short(), std::true_type()) : launch(short(), std::false_type());
}

}  // namespace
