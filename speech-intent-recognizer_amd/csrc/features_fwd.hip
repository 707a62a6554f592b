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
// pair of features_gen.hip (feat_gen_frames_kernel + feat_gen_norm_kernel).  Its gradient is features_bwd.hip; the three share
// feat_common.h (sample loads, host dispatch), feat_lds.h (the LDS layouts) and wave_fft.h (the in-wave FFT primitives).
#include "feat_common.h"

namespace {

template <typename WT, bool AUG>
__global__ __launch_bounds__(THREADS) void feat_utt_kernel(
    const WT* __restrict__ wave, long long wave_stride, const int32_t* __restrict__ lengths, int max_len,
    float* __restrict__ out, float* __restrict__ db_out, int t_pad, FeatTables tb, AugArgs aug,
    const int32_t* __restrict__ time_mask, const int32_t* __restrict__ freq_mask) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const FeatUttLds lay(tb.mel_nnz);
    float* lds = reinterpret_cast<float*>(smem);
    cf32* xall = reinterpret_cast<cf32*>(lds + lay.xall);
    double* red = reinterpret_cast<double*>(lds + lay.red);
    float* Pbuf = lds + lay.pbuf;
    float* melw = lds + lay.melw;
    float* tail = melw + lay.melw_pad;
    cf32* winl = reinterpret_cast<cf32*>(tail + lay.winl);
    cf32* twul = reinterpret_cast<cf32*>(tail + lay.twul);
    cf32* tw2l = reinterpret_cast<cf32*>(tail + lay.tw2l);

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
                // (twin of fft512, feat_common.h, with the pass-1 twiddles in registers: through fft512 this kernel takes 128 VGPRs, not 124)
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

}  // namespace

extern "C" size_t sir_features_workspace_bytes(const sir_handle* h, int batch, int max_len) {
    if (batch <= 0 || max_len <= 0) return 0;
    if (h && h->general) return sir_features_gen_slab_bytes(h, batch, max_len);     // the launch pair's dB slab: every frame of every clip
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
    const size_t esz = sir_wave_elem_bytes(wave_dtype);
    if (!esz) { sir_set_error("sir_features_fwd: wave_dtype %d", wave_dtype); return SIR_EINVAL; }
    if (workspace_bytes < sir_features_workspace_bytes(h, batch, max_len)) { sir_set_error("sir_features_fwd: workspace too small"); return SIR_ENOMEM; }
    if (((uintptr_t)wave % esz) != 0) { sir_set_error("sir_features_fwd: waveform pointer is not aligned to its sample type"); return SIR_EINVAL; }
    if (h->general) {
        if (((uintptr_t)workspace % 16) != 0) { sir_set_error("sir_features_fwd: the workspace is not 16-byte aligned"); return SIR_EINVAL; }
        SIR_TRY(sir_features_gen_launch(h, wave, wave_dtype, wave_stride, lengths, batch, max_len, out, t_pad, db_out, workspace, aug, stream));
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
    const AugHost a(aug);
    const size_t lds = FeatUttLds(h->mel_nnz).bytes();
    dim3 grid(batch), block(THREADS);
    {
    SirProfScope prof(h, SIR_K_FEAT_FRAMES, stream);
    SIR_TRY(dispatch_wave(wave_dtype, a.wave_aug, [&](auto ty, auto augf) {
        using TY = decltype(ty);
        constexpr bool AUGF = decltype(augf)::value;
        SIR_TRY(sir_lds_opt_in(h, (const void*)feat_utt_kernel<TY, AUGF>, (int)lds));       // (> 64 KB of dynamic LDS needs the opt-in)
        hipLaunchKernelGGL((feat_utt_kernel<TY, AUGF>), grid, block, lds, stream, (const TY*)wave, (long long)wave_stride, lengths,
                           max_len, out, db_out, t_pad, tb, a.ag, a.tmask, a.fmask);
        return (int)SIR_OK;
    }));
    }
    SIR_HIP_TRY(hipGetLastError());
    return SIR_OK;
}
