// General forward path (sir_features_fwd): every front-end but n_fft 1024 / hop 512 / win_length 1024.
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
#include "feat_common.h"

namespace {

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
    const FeatGenLds lay(R1, tb.mel_nnz);
    float* lds = reinterpret_cast<float*>(smem);
    cf32* xall = reinterpret_cast<cf32*>(lds + lay.xall);             // [NW][XB]
    float* Pbuf = lds + lay.pbuf;                                      // [2][NW][PR]
    float* melw = lds + lay.melw;
    float* tail = melw + lay.melw_pad;
    cf32* winl = reinterpret_cast<cf32*>(tail + lay.winl);
    cf32* twnl = reinterpret_cast<cf32*>(tail + lay.twnl);
    cf32* twul = reinterpret_cast<cf32*>(tail + lay.twul);

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
            float acc = 0.0f;                                          // (twin of feat_utt_kernel's mel chain, features_fwd.hip)
            for (int i = 0; i < md.z; ++i) acc = fmaf(wr[i], pr[i], acc);
            srow[(size_t)md.x * slab_t + tm] = (acc <= AMIN) ? -100.0f : 10.0f * log10f(acc);
        }
    }
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
        mean = (float)(block_sum(s, red, lane, wv) / cnt);
        double q2 = 0.0;
        for (int f = wv; f < n_mels; f += NW)
            for (int t = lane; t < T; t += 64) { const float d = srow[(size_t)f * slab_t + t] - mean; q2 += (double)(d * d); }
        const double m2 = block_sum(q2, red, lane, wv);
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
    const AugHost a(aug);
    float* slab = reinterpret_cast<float*>(workspace);
    dim3 grid(batch, tiles), block(THREADS);
    SirProfScope prof(h, SIR_K_FEAT_FRAMES, stream);                   // the pair is timed under the one id
    SIR_TRY(dispatch_wave(wave_dtype, a.wave_aug, [&](auto ty, auto augf) {
        using TY = decltype(ty);
        constexpr bool AUGF = decltype(augf)::value;
        SIR_TRY(sir_lds_opt_in(h, (const void*)feat_gen_frames_kernel<TY, AUGF, R1>, (int)lds));
        hipLaunchKernelGGL((feat_gen_frames_kernel<TY, AUGF, R1>), grid, block, lds, stream, (const TY*)wave,
                           (long long)wave_stride, lengths, max_len, slab, slab_t, tb, a.ag);
        return (int)SIR_OK;
    }));
    hipLaunchKernelGGL(feat_gen_norm_kernel, dim3(batch), block, 0, stream, slab, slab_t, lengths, max_len, N, hop,
                       h->cfg.n_mels, out, db_out, t_pad, a.tmask, a.fmask);
    return SIR_OK;
}

}  // namespace

size_t sir_features_gen_slab_bytes(const sir_handle* h, int batch, int max_len) {
    return sir_align_up((size_t)batch * h->cfg.n_mels * (size_t)(1 + max_len / h->cfg.hop_length) * sizeof(float), 256);
}

// dynamic LDS of feat_gen_frames_kernel<.., n_fft / 128> (feat_lds.h)
size_t sir_features_gen_lds_bytes(int n_fft, int mel_nnz) { return FeatGenLds(n_fft / 128, mel_nnz).bytes(); }

int sir_features_gen_launch(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride, const int32_t* lengths, int batch,
                            int max_len, float* out, int t_pad, float* db_out, void* workspace, const sir_augment* aug,
                            hipStream_t stream) {
    switch (h->cfg.n_fft) {
        case 256: return launch_gen<2>(h, wave, wave_dtype, wave_stride, lengths, batch, max_len, out, t_pad, db_out, workspace, aug, stream);
        case 512: return launch_gen<4>(h, wave, wave_dtype, wave_stride, lengths, batch, max_len, out, t_pad, db_out, workspace, aug, stream);
        default:  return launch_gen<8>(h, wave, wave_dtype, wave_stride, lengths, batch, max_len, out, t_pad, db_out, workspace, aug, stream);
    }
}
