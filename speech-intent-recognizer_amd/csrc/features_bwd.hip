// Gradient of the feature path with respect to the waveform (sir_features_bwd), n_fft 1024 / hop 512 / win_length 1024.
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
#include "feat_common.h"

namespace {

struct MelTap { int fa; float wa; int fb; float wb; };      // the (at most) two filters that cover an FFT bin, ascending; weight 0 = none
static_assert(sizeof(MelTap) == 4 * FEAT_MELTAP && SIR_NFREQ <= MEL_TAPS, "feat_lds.h: the tap table");
constexpr float DB_SCALE = 4.34294481903251827651f;       // 10 / ln 10

template <typename WT, bool AUG>
__global__ __launch_bounds__(THREADS) void feat_utt_bwd_kernel(
    const WT* __restrict__ wave, long long wave_stride, const int32_t* __restrict__ lengths, int max_len,
    const float* __restrict__ db, const float* __restrict__ dout, int t_pad, FeatTables tb, const MelTap* __restrict__ taps,
    AugArgs aug, const int32_t* __restrict__ time_mask, const int32_t* __restrict__ freq_mask,
    float* __restrict__ dwave, long long dwave_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const FeatUttBwdLds lay(tb.mel_nnz);
    float* lds = reinterpret_cast<float*>(smem);
    cf32* xall = reinterpret_cast<cf32*>(lds + lay.xall);             // (after step 3: [NW][1024] frame gradients)
    double* red = reinterpret_cast<double*>(lds + lay.red);
    float* P = lds + lay.p;
    float* dmt = lds + lay.dmt;
    float* carry = lds + lay.carry;
    MelTap* tapl = reinterpret_cast<MelTap*>(lds + lay.tapl);
    float* melw = lds + lay.melw;
    float* tail = melw + lay.melw_pad;
    cf32* winl = reinterpret_cast<cf32*>(tail + lay.winl);
    cf32* twul = reinterpret_cast<cf32*>(tail + lay.twul);
    cf32* tw2l = reinterpret_cast<cf32*>(tail + lay.tw2l);
    cf32* tw1l = reinterpret_cast<cf32*>(tail + lay.tw1l);

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
    if (tid < 512) {                                                   // (twin of feat_utt_kernel's table staging, features_fwd.hip)
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
            float* prow = P + wv * PROW;                               // (twin of feat_utt_kernel's untangle, features_fwd.hip; keeps X)
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
                float acc = 0.0f;                                      // (twin of feat_utt_kernel's mel chain, features_fwd.hip)
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

}  // namespace

int sir_features_bwd_launch(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride, const int32_t* lengths,
                            int batch, int max_len, const float* db, const float* dout, int t_pad, const sir_augment* aug,
                            float* dwave, int64_t dwave_stride, hipStream_t stream) {
    if (!h || !wave || !lengths || !db || !dout || !dwave) { sir_set_error("sir_features_bwd: NULL argument"); return SIR_EINVAL; }
    if (batch <= 0 || max_len <= 0 || t_pad <= 0 || wave_stride < max_len || dwave_stride < max_len) {
        sir_set_error("sir_features_bwd: bad shape batch=%d max_len=%d t_pad=%d wave_stride=%lld dwave_stride=%lld", batch, max_len,
                      t_pad, (long long)wave_stride, (long long)dwave_stride);
        return SIR_EINVAL;
    }
    const size_t esz = sir_wave_elem_bytes(wave_dtype);
    if (!esz) { sir_set_error("sir_features_bwd: wave_dtype %d", wave_dtype); return SIR_EINVAL; }
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
    const AugHost a(aug);
    const MelTap* taps = reinterpret_cast<const MelTap*>(h->mel_taps);
    const size_t lds = FeatUttBwdLds(h->mel_nnz).bytes();
    dim3 grid(batch), block(THREADS);
    // (no SirProfScope: the profile id tables are closed; devtools/feat_only.py --backward times this launch with events)
    SIR_TRY(dispatch_wave(wave_dtype, a.wave_aug, [&](auto ty, auto augf) {
        using TY = decltype(ty);
        constexpr bool AUGF = decltype(augf)::value;
        SIR_TRY(sir_lds_opt_in(h, (const void*)feat_utt_bwd_kernel<TY, AUGF>, (int)lds));
        hipLaunchKernelGGL((feat_utt_bwd_kernel<TY, AUGF>), grid, block, lds, stream, (const TY*)wave, (long long)wave_stride, lengths,
                           max_len, db, dout, t_pad, tb, taps, a.ag, a.tmask, a.fmask, dwave, (long long)dwave_stride);
        return (int)SIR_OK;
    }));
    SIR_HIP_TRY(hipGetLastError());
    return SIR_OK;
}
