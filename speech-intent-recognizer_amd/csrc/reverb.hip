// Room reverberation and background noise at a chosen SNR, ahead of the feature path (sir_wave_reverb_mix; the reference
// has neither effect: its augment.py stops at Gaussian noise of a fixed sigma).
//
// Per row b (L = lengths[b] clamped to [0, max_len], x = the row's samples, PCM16 dequantised as s / 32768):
//   reverb  y[n] = sum_{k < min(K, n + 1)} x[n - k] h_r[k], n in [0, L): the head of the linear convolution with RIR r (K taps);
//           the tail beyond L is dropped, the RIR is used as given; r = -1: y = x, a copy.
//   noise   out[n] = y[n] + g v[(o + n) mod M], g = sqrt(P_y / (P_v 10^(snr_db / 10))), P_y = mean y^2 over [0, L), P_v = mean
//           square of the L noise samples actually used; g = 0 when P_y or P_v is 0; v = -1: out = y, a copy.
//   out[b] is zero on [L, max_len).  A bad row (an index or a bank length out of range, a non-finite snr_db, a g that is no
//   finite float32) is zero on [0, max_len) with gain 0 and raises SIR_STATUS_REVERB.
//
// reverb_mix_kernel: ONE 256-thread workgroup (4 waves) per row.  Direct form costs L x K multiply-adds (4e8 per 3 s clip at K =
// 8192), so the convolution is uniformly partitioned overlap-save on the 1024-point real FFT: the RIR is cut into P =
// ceil(K / 512) partitions of 512 taps, each zero-padded to 1024 and transformed once per row (H_p, held in LDS, pre-scaled by
// 1/1024); output block m (512 samples) is the second half of IFFT(sum_{p <= min(P - 1, m)} H_p X_{m-p}) where X_j is the
// spectrum of the input window [512 (j - 1), 512 (j + 1)).  Neither the X_j nor the blocks depend on each other, so the four
// waves work on four consecutive blocks at once ("round"): each transforms its window and stores X_j in an LDS ring of P + 3
// spectra, one barrier, each multiply-accumulates its block's spectrum from the ring and H, transforms back and stores 512
// samples, one barrier.  A transform is a 512-point complex FFT of the sample pairs inside ONE wave (three radix-8 passes,
// two exchanges through the wave's private LDS slab, no workgroup barrier: the scheme and the slab layouts of the feature kernels, over wave_fft.h)
// plus the real-FFT untangle; a spectrum is kept as 512 complex values, slot 0 holding the two real bins (X[0], X[512]).
// LDS: 4 KB x (2 P + 3) + 18 KB of slabs = 158 KB at P = 16 (of 160 KB: one workgroup per CU), 42 KB at P = 2.
// The noise stage follows in the same workgroup: y is in `out`, the threads re-read it (their own workgroup's stores, fenced)
// together with the wrapped noise samples, reduce sum y^2 and sum v^2 in a fixed order (per-thread float, wave shuffles, the
// four wave sums combined in double: no atomics, bit-reproducible, a function of the row alone), and add g v in a second sweep.
// HBM traffic per row (algorithmic): L x 4 B read (2 for PCM16) + K x 4 B + L x 4 B of noise + L x 4 B written.
#include <math.h>
#include <stdint.h>
#include "sir_internal.h"
#include "wave_fft.h"
#include "wave_sample.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * SIR_WAVE;
constexpr int kPart = 512;             // taps per RIR partition = samples per output block
constexpr int kMaxRir = 8192;
constexpr int kMaxParts = kMaxRir / kPart;
constexpr int kRingExtra = kWaves - 1; // ring slots beyond the partitions: a round's four spectra land before the oldest is dropped
constexpr int kSlab = 8 * XS;          // complex slots of a wave's slab

__device__ __forceinline__ cf32 cconj(cf32 a) { return cf32{a.x, -a.y}; }
__device__ __forceinline__ cf32 mul_pi(cf32 a) { return cf32{-a.y, a.x}; }                       // a * (+i)
// the lane's twiddles: t1[k] = W512^(lane k), t2[k] = W64^((lane & 7) k), tu[j] = W1024^(lane + 64 j)
struct Twiddles { cf32 t1[8], t2[8], tu[8]; };

// 512-point complex DFT inside one wave: on entry the lane holds points lane + 64 j, on return bins lane + 64 j.
__device__ __forceinline__ void fft512(cf32 (&v)[8], const Twiddles& tw, cf32* xb, int lane) {
    dft8(v);                                    // pass 1: over n2 (stride 64), twiddle W512^(n1 k2)
#pragma unroll
    for (int k = 1; k < 8; ++k) v[k] = cmul(v[k], tw.t1[k]);
    wave_fence();
#pragma unroll
    for (int k = 0; k < 8; ++k) xb[k * XS + lane] = v[k];
    wave_fence();
    const int k2 = lane >> 3, m1 = lane & 7;    // pass 2: lane = (k2, m1): over m2, twiddle W64^(m1 j2)
#pragma unroll
    for (int m = 0; m < 8; ++m) v[m] = xb[k2 * XS + m1 + 8 * m];
    dft8(v);
#pragma unroll
    for (int k = 1; k < 8; ++k) v[k] = cmul(v[k], tw.t2[k]);
    wave_fence();
#pragma unroll
    for (int j = 0; j < 8; ++j) xb[ex2_index(k2, j, m1)] = v[j];
    wave_fence();
#pragma unroll
    for (int m = 0; m < 8; ++m) v[m] = xb[ex2_index(lane & 7, lane >> 3, m)];   // pass 3: lane = k2 + 8 j2: over m1
    dft8(v);
}

// v[j] = Z[k] -> part[j] = Z[(512 - k) & 511], k = lane + 64 j, through the wave's slab
__device__ __forceinline__ void partners(const cf32 (&v)[8], cf32 (&part)[8], cf32* xb, int lane) {
    wave_fence();
#pragma unroll
    for (int j = 0; j < 8; ++j) xb[lane + 64 * j] = v[j];
    wave_fence();
#pragma unroll
    for (int j = 0; j < 8; ++j) part[j] = xb[(512 - lane - 64 * j) & 511];
    wave_fence();
}

// 1024 real samples, packed as v[j] = (s[2 n], s[2 n + 1]), n = lane + 64 j -> spectrum slots k = lane + 64 j times `scale`:
// slot k >= 1 = X[k], slot 0 = (X[0], X[512]) (both real)
__device__ __forceinline__ void rfft1024(cf32 (&v)[8], const Twiddles& tw, cf32* xb, int lane, float scale) {
    fft512(v, tw, xb, lane);
    cf32 zp[8];
    partners(v, zp, xb, lane);
    const float hs = 0.5f * scale;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const cf32 z = v[j], c = cconj(zp[j]);
        // X[k] = (Z[k] + conj Z[512-k]) / 2 - i W1024^k (Z[k] - conj Z[512-k]) / 2
        v[j] = ((z + c) + mul_mi(cmul(tw.tu[j], z - c))) * hs;
        if (j == 0 && lane == 0) v[0] = cf32{z.x + z.y, z.x - z.y} * scale;
    }
}

// inverse of rfft1024 without its 1/1024: spectrum slots v[j] -> v[j] = (s[2 n], s[2 n + 1]) * 1024, n = lane + 64 j
__device__ __forceinline__ void irfft1024(cf32 (&v)[8], const Twiddles& tw, cf32* xb, int lane) {
    cf32 yp[8];
    partners(v, yp, xb, lane);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const cf32 y = v[j], c = cconj(yp[j]);
        // Z'[k] = (Y[k] + conj Y[512-k]) + i cconj(W1024^k) (Y[k] - conj Y[512-k]); handed to the forward transform conjugated
        cf32 z = (y + c) + mul_pi(cmul(cconj(tw.tu[j]), y - c));
        if (j == 0 && lane == 0) z = cf32{y.x + y.y, y.x - y.y};
        v[j] = cconj(z);
    }
    fft512(v, tw, xb, lane);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = cconj(v[j]);
}

struct ReverbArgs {
    const float* rir_bank; long long rir_stride; const int* rir_lengths; int n_rir, max_rir_len; const int* rir_index;
    const float* noise_bank; long long noise_stride; const int* noise_lengths; int n_noise; const int* noise_index;
    const int* noise_offset; const float* snr_db;
    const float2* tw512; const float2* tw1024;
    int parts;                 // partitions the LDS is sized for: ceil(max_rir_len / 512), 0 without reverb
};

template <typename WT>
__global__ __launch_bounds__(kThreads) void reverb_mix_kernel(const WT* __restrict__ wave, long long wave_stride, const int* __restrict__ lengths,
                                                              int max_len, ReverbArgs a, float* __restrict__ out, long long out_stride,
                                                              float* __restrict__ gain, unsigned int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* red = reinterpret_cast<double*>(smem);                     // [2][kWaves] + the gain + its bad-row flag
    cf32* slabs = reinterpret_cast<cf32*>(red + 2 * kWaves + 2);       // [kWaves][kSlab]
    cf32* Hs = slabs + kWaves * kSlab;                                 // [parts][512]
    cf32* ring = Hs + a.parts * 512;                                   // [parts + kRingExtra][512]

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (SIR_WAVE - 1), wv = tid / SIR_WAVE;
    int L = lengths ? lengths[b] : max_len;
    L = L < 0 ? 0 : (L > max_len ? max_len : L);
    const WT* x = wave + (size_t)b * wave_stride;
    float* y = out + (size_t)b * out_stride;

    // per-row arguments (block-uniform); a bank length is read only behind a valid index
    bool bad = false;
    const int r = a.rir_index ? a.rir_index[b] : -1;
    int K = 0;
    if (r < -1 || r >= a.n_rir) bad = true;
    else if (r >= 0) { K = a.rir_lengths[r]; bad = K < 1 || K > a.max_rir_len; }
    const int nv = a.noise_index ? a.noise_index[b] : -1;
    int M = 0;
    float snr = 0.0f;
    if (nv < -1 || nv >= a.n_noise) bad = true;
    else if (nv >= 0) {
        M = a.noise_lengths[nv];
        snr = a.snr_db[b];
        if (M < 1 || (long long)M > a.noise_stride || !(fabsf(snr) <= 3.0e38f)) bad = true;
    }
    if (bad) {
        if (tid == 0) {
            __hip_atomic_fetch_or(status, SIR_STATUS_REVERB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            gain[b] = 0.0f;
        }
        for (int i = tid; i < max_len; i += kThreads) y[i] = 0.0f;
        return;
    }
    for (int i = L + tid; i < max_len; i += kThreads) y[i] = 0.0f;

    if (r < 0) {
        for (int i = tid; i < L; i += kThreads) y[i] = to_f32<WT>(x[i]);
    } else {
        const float* h = a.rir_bank + (size_t)r * a.rir_stride;
        const int P = (K + kPart - 1) / kPart;
        const int R = a.parts + kRingExtra;
        cf32* xb = slabs + wv * kSlab;
        Twiddles tw;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            tw.t1[k] = CF(a.tw512[(lane * k) & 511]);
            tw.t2[k] = CF(a.tw512[(8 * (lane & 7) * k) & 511]);
            tw.tu[k] = CF(a.tw1024[lane + 64 * k]);
        }
        cf32 v[8];
        for (int p = wv; p < P; p += kWaves) {                           // H_p: taps [512 p, 512 p + 512), zero-padded to 1024
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i0 = kPart * p + 2 * (lane + 64 * j);
                v[j].x = (j < 4 && i0 < K) ? h[i0] : 0.0f;
                v[j].y = (j < 4 && i0 + 1 < K) ? h[i0 + 1] : 0.0f;
            }
            rfft1024(v, tw, xb, lane, 1.0f / 1024.0f);
#pragma unroll
            for (int j = 0; j < 8; ++j) Hs[p * 512 + lane + 64 * j] = v[j];
        }
        const int nblk = (L + kPart - 1) / kPart;
        const int nrounds = (nblk + kWaves - 1) / kWaves;
        for (int rd = 0; rd < nrounds; ++rd) {
            const int m = kWaves * rd + wv;
            if (m < nblk) {                                              // X_m of the window [512 (m - 1), 512 (m + 1))
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int i0 = kPart * (m - 1) + 2 * (lane + 64 * j);
                    v[j].x = (i0 >= 0 && i0 < L) ? to_f32<WT>(x[i0]) : 0.0f;
                    v[j].y = (i0 + 1 >= 0 && i0 + 1 < L) ? to_f32<WT>(x[i0 + 1]) : 0.0f;
                }
                rfft1024(v, tw, xb, lane, 1.0f);
                cf32* slot = ring + (m % R) * 512;
#pragma unroll
                for (int j = 0; j < 8; ++j) slot[lane + 64 * j] = v[j];
            }
            __syncthreads();                                             // the round's spectra (and, in round 0, every H_p) are in LDS
            if (m < nblk) {
                cf32 acc[8], acc0 = cf32{0.0f, 0.0f};
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = cf32{0.0f, 0.0f};
                const int np = m + 1 < P ? m + 1 : P;                    // X_j = 0 for j < 0
                int s = m % R;
                for (int p = 0; p < np; ++p) {
                    const cf32* hp = Hs + p * 512 + lane;
                    const cf32* xp = ring + s * 512 + lane;
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] += cmul(hp[64 * j], xp[64 * j]);
                    acc0 += hp[0] * xp[0];                               // slot 0 of lane 0: two real bins, element by element
                    s = s == 0 ? R - 1 : s - 1;
                }
                if (lane == 0) acc[0] = acc0;
                irfft1024(acc, tw, xb, lane);
#pragma unroll
                for (int j = 4; j < 8; ++j) {                            // second half of the 1024 samples = block m
                    const int i0 = kPart * m + 2 * (lane + 64 * (j - 4));
                    if (i0 < L) y[i0] = acc[j].x;
                    if (i0 + 1 < L) y[i0 + 1] = acc[j].y;
                }
            }
            __syncthreads();                                             // before the next round overwrites the oldest slots
        }
    }

    if (nv < 0) {
        if (tid == 0) gain[b] = 0.0f;
        return;
    }
    // noise at the chosen SNR: y is in `out`, written by this workgroup
    __threadfence();
    __syncthreads();
    __threadfence();
    const float* vn = a.noise_bank + (size_t)nv * a.noise_stride;
    long long o = (long long)a.noise_offset[b] % (long long)M;
    if (o < 0) o += M;
    const unsigned o0 = (unsigned)o, Mu = (unsigned)M;
    float sy = 0.0f, sv = 0.0f;
    for (int i = tid; i < L; i += kThreads) {
        const float yy = y[i], vv = vn[(o0 + (unsigned)i) % Mu];
        sy = fmaf(yy, yy, sy);
        sv = fmaf(vv, vv, sv);
    }
    sy = wave_sum(sy);
    sv = wave_sum(sv);
    if (lane == 0) { red[wv] = (double)sy; red[kWaves + wv] = (double)sv; }
    __syncthreads();
    if (tid == 0) {
        double Sy = 0.0, Sv = 0.0;
        for (int i = 0; i < kWaves; ++i) { Sy += red[i]; Sv += red[kWaves + i]; }
        double g = 0.0;
        if (Sy > 0.0 && Sv > 0.0) g = sqrt(Sy / (Sv * pow(10.0, (double)snr / 10.0)));   // the 1 / L of both means cancels
        float gf = (float)g;
        // an extreme finite snr_db (10^(snr / 10) underflows to 0 below about -3240 dB, g passes FLT_MAX below about -770 dB
        // at ordinary levels) gives a gain that is no finite float32: a bad row, as a NaN snr_db is
        const bool inf_gain = !(fabsf(gf) <= 3.4028234e38f);
        if (inf_gain) {
            __hip_atomic_fetch_or(status, SIR_STATUS_REVERB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            gf = 0.0f;
        }
        gain[b] = gf;
        red[2 * kWaves] = (double)gf;
        red[2 * kWaves + 1] = inf_gain ? 1.0 : 0.0;
    }
    __syncthreads();
    if (red[2 * kWaves + 1] != 0.0) {                                    // block-uniform
        for (int i = tid; i < L; i += kThreads) y[i] = 0.0f;
        return;
    }
    const float g = (float)red[2 * kWaves];
    for (int i = tid; i < L; i += kThreads) y[i] = fmaf(g, vn[(o0 + (unsigned)i) % Mu], y[i]);
}

size_t lds_bytes(int parts) {
    return (2 * kWaves + 2) * sizeof(double) + (size_t)(kWaves * kSlab + (parts ? (2 * parts + kRingExtra) * 512 : 0)) * sizeof(cf32);
}

size_t ws_bytes(int batch) { return sir_align_up((size_t)batch * sizeof(float), 256); }

bool overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}

}  // namespace

extern "C" size_t sir_reverb_workspace_bytes(const sir_handle* h, int batch, int max_len, int max_rir_len) {
    if (!h || batch <= 0 || max_len <= 0 || max_rir_len < 0 || max_rir_len > kMaxRir) return 0;
    return ws_bytes(batch);
}

extern "C" int sir_wave_reverb_mix(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride, const int32_t* lengths, int batch,
                                   int max_len, const float* rir_bank, int64_t rir_stride, const int32_t* rir_lengths, int n_rir,
                                   int max_rir_len, const int32_t* rir_index, const float* noise_bank, int64_t noise_stride,
                                   const int32_t* noise_lengths, int n_noise, const int32_t* noise_index, const int32_t* noise_offset,
                                   const float* snr_db, float* out, int64_t out_stride, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    if (!h || !wave || !out) { sir_set_error("sir_wave_reverb_mix: NULL argument"); return SIR_EINVAL; }
    if (batch <= 0 || batch > 65535 || max_len <= 0 || wave_stride < max_len || out_stride < max_len) {
        sir_set_error("sir_wave_reverb_mix: bad sizes (batch %d, max_len %d, wave_stride %lld, out_stride %lld)", batch, max_len,
                      (long long)wave_stride, (long long)out_stride);
        return SIR_EINVAL;
    }
    if (!sir_wave_elem_bytes(wave_dtype)) { sir_set_error("sir_wave_reverb_mix: bad wave_dtype %d", wave_dtype); return SIR_EINVAL; }
    if (rir_index) {
        if (max_rir_len < 1 || max_rir_len > kMaxRir) {
            sir_set_error("sir_wave_reverb_mix: max_rir_len %d is outside [1, %d]", max_rir_len, kMaxRir);
            return SIR_EINVAL;
        }
        if (!rir_bank || !rir_lengths || n_rir < 1 || rir_stride < max_rir_len) {
            sir_set_error("sir_wave_reverb_mix: rir_index needs a bank (n_rir %d, rir_stride %lld, max_rir_len %d)", n_rir, (long long)rir_stride, max_rir_len);
            return SIR_EINVAL;
        }
    }
    if (noise_index && (!noise_bank || !noise_lengths || !noise_offset || !snr_db || n_noise < 1 || noise_stride < 1 || noise_stride > 0x7fffffffLL)) {
        sir_set_error("sir_wave_reverb_mix: noise_index needs a bank, offsets and SNRs (n_noise %d, noise_stride %lld)", n_noise, (long long)noise_stride);
        return SIR_EINVAL;
    }
    const size_t wbytes = sir_wave_elem_bytes(wave_dtype);
    if (overlap(wave, ((size_t)(batch - 1) * wave_stride + max_len) * wbytes, out, ((size_t)(batch - 1) * out_stride + max_len) * sizeof(float))) {
        sir_set_error("sir_wave_reverb_mix: out overlaps wave (the convolution reads samples behind the ones it writes)");
        return SIR_EINVAL;
    }
    const size_t need = ws_bytes(batch);
    if (!workspace || workspace_bytes < need || (uintptr_t)workspace % 256 != 0) {
        sir_set_error("sir_wave_reverb_mix: workspace of %zu bytes at %p, need %zu bytes, 256-byte aligned", workspace_bytes, workspace, need);
        return SIR_ENOMEM;
    }
    ReverbArgs a;
    a.rir_bank = rir_bank; a.rir_stride = (long long)rir_stride; a.rir_lengths = rir_lengths; a.n_rir = rir_index ? n_rir : 0;
    a.max_rir_len = max_rir_len; a.rir_index = rir_index;
    a.noise_bank = noise_bank; a.noise_stride = (long long)noise_stride; a.noise_lengths = noise_lengths; a.n_noise = noise_index ? n_noise : 0;
    a.noise_index = noise_index; a.noise_offset = noise_offset; a.snr_db = snr_db;
    a.tw512 = h->tw512; a.tw1024 = h->tw1024;
    a.parts = rir_index ? (max_rir_len + kPart - 1) / kPart : 0;
    const size_t lds = lds_bytes(a.parts);
    hipStream_t st = (hipStream_t)stream;
    return sir_wave_dispatch(wave_dtype, [&](auto tag) {
        using WT = decltype(tag);
        SIR_TRY(sir_lds_opt_in(h, (const void*)reverb_mix_kernel<WT>, (int)lds_bytes(kMaxParts)));
        hipLaunchKernelGGL(reverb_mix_kernel<WT>, dim3(batch), dim3(kThreads), lds, st, (const WT*)wave, (long long)wave_stride, lengths, max_len, a,
                           out, (long long)out_stride, (float*)workspace, h->status);
        return sir_check_hip(hipGetLastError(), "reverb_mix_kernel");
    });
}
