// Dynamic-LDS layout of the three frame kernels of the feature path: feat_utt_kernel (features_fwd.hip), feat_utt_bwd_kernel
// (features_bwd.hip) and feat_gen_frames_kernel (features_gen.hip).  Stated once, here: the kernel takes its region pointers from
// the struct, the launch site takes .bytes(), and tests/test_feat_lds_layout_host.py reads it with the host compiler -- so no HIP
// header is included and nothing below is device-only.  The kernels index every region up to its last word: a region is added or
// resized HERE, never on one side.
#pragma once
#include <stddef.h>

#ifdef __HIPCC__
#define FEAT_LDS_FN __host__ __device__ inline
#else
#define FEAT_LDS_FN inline
#endif

constexpr int NW = 16;           // waves per workgroup = frames per round
constexpr int XBUF = 8 * 72;     // complex slots of a wave's exchange slab: the 8 rows of the first exchange (XS, wave_fft.h)
constexpr int PROW = 514;        // words per power-spectrum row: the 16 frames of a filter sit on 16 different banks
constexpr int TW2S = 10;         // row stride (complex) of the pass-2 twiddle table in LDS
constexpr int DMS = 65;          // row stride of the backward's dM tile: the 16 frames a filter's threads write fall on 16 banks
constexpr int MEL_TAPS = 516;    // entries of the backward's tap table: the 513 bins, rounded up
// Offsets and sizes below count 4-byte LDS WORDS (every region is whole words).  One region has a run-time size, the filter weights;
// the regions behind it are offsets from its end, so that a kernel forms `melw + melw_pad` once and reaches them at compile-time
// distances from that pointer -- the addresses, and the instructions, of the carve each kernel used to spell out.
constexpr int FEAT_CF32 = 2, FEAT_F64 = 2, FEAT_MELTAP = 4;   // words of a complex value, a double, a tap entry (MelTap, features_bwd.hip)

// the next `words` of the workgroup's LDS: returns their offset and moves `at` behind them
FEAT_LDS_FN int feat_lds_take(int& at, int words) { const int o = at; at += words; return o; }
// filter weights are padded to whole float4s, so that what follows keeps 16-byte alignment
FEAT_LDS_FN int feat_lds_melw_words(int mel_nnz) { return (mel_nnz + 3) & ~3; }

struct FeatLds {                 // what the three layouts have in common
    int melw, melw_pad;          // float [mel_nnz] filter weights and the words they take; what follows counts from tail(), their end
    int words;                   // the whole of it
    FEAT_LDS_FN int tail() const { return melw + melw_pad; }
    FEAT_LDS_FN size_t bytes() const { return (size_t)words * 4; }
};

struct FeatUttLds : FeatLds {    // feat_utt_kernel; word offsets, regions in this order
    int xall, red, pbuf, winl, twul, tw2l;
    FEAT_LDS_FN explicit FeatUttLds(int mel_nnz) {
        int at = 0;
        xall = feat_lds_take(at, NW * XBUF * FEAT_CF32);       // cf32 [NW][XBUF] exchange slabs
        red = feat_lds_take(at, NW * FEAT_F64);                // double [NW] reduction scratch
        pbuf = feat_lds_take(at, 2 * NW * PROW);               // float [2][NW][PROW] power spectra, by round parity
        melw = at; melw_pad = feat_lds_melw_words(mel_nnz); at = 0;
        winl = feat_lds_take(at, 512 * FEAT_CF32);             // cf32 [512] Hann window as sample pairs
        twul = feat_lds_take(at, 512 * FEAT_CF32);             // cf32 [512] -i/2 * W1024^k, the untangle twiddles
        tw2l = feat_lds_take(at, 8 * TW2S * FEAT_CF32);        // cf32 [8][TW2S] W64^(m1 * j2), row m1 (stride 10: the 8 rows' 16-byte reads fall on disjoint banks)
        words = tail() + at;
    }
};

struct FeatUttBwdLds : FeatLds { // feat_utt_bwd_kernel
    int xall, red, p, dmt, carry, tapl, winl, twul, tw2l, tw1l;
    FEAT_LDS_FN explicit FeatUttBwdLds(int mel_nnz) {
        int at = 0;
        xall = feat_lds_take(at, NW * XBUF * FEAT_CF32);       // cf32 [NW][XBUF] exchange slabs; after step 3: [NW][1024] frame gradients
        red = feat_lds_take(at, NW * FEAT_F64);                // double [NW] reduction scratch
        p = feat_lds_take(at, NW * PROW);                      // float [NW][PROW] power spectra of the round
        dmt = feat_lds_take(at, NW * DMS);                     // float [NW][DMS] dM of the round
        carry = feat_lds_take(at, 512);                        // float [512] second half of the previous round's last frame
        tapl = feat_lds_take(at, MEL_TAPS * FEAT_MELTAP);      // MelTap [513 (+3)]
        melw = at; melw_pad = feat_lds_melw_words(mel_nnz); at = 0;
        winl = feat_lds_take(at, 512 * FEAT_CF32);             // cf32 [512] Hann window as sample pairs
        twul = feat_lds_take(at, 512 * FEAT_CF32);             // cf32 [512] -i/2 * W1024^k
        tw2l = feat_lds_take(at, 8 * TW2S * FEAT_CF32);        // cf32 [8][TW2S]
        tw1l = feat_lds_take(at, 8 * 64 * FEAT_CF32);          // cf32 [8][64] W512^(lane * k), row k (16 registers the spectrum needs here)
        words = tail() + at;
    }
};

struct FeatGenLds : FeatLds {    // feat_gen_frames_kernel<.., R1>: n_fft = 128 R1, N = 64 R1 packed complex points
    int xall, pbuf, winl, twnl, twul;
    FEAT_LDS_FN FeatGenLds(int r1, int mel_nnz) {
        const int n = 64 * r1;
        int at = 0;
        xall = feat_lds_take(at, NW * r1 * (XBUF / 8) * FEAT_CF32);   // cf32 [NW][R1 * XS] exchange slabs (XS = XBUF / 8)
        pbuf = feat_lds_take(at, 2 * NW * (n + 2));            // float [2][NW][N + 2] power spectra, by round parity
        melw = at; melw_pad = feat_lds_melw_words(mel_nnz); at = 0;
        winl = feat_lds_take(at, n * FEAT_CF32);               // cf32 [N] window as sample pairs
        twnl = feat_lds_take(at, n * FEAT_CF32);               // cf32 [N] W_N^k
        twul = feat_lds_take(at, n * FEAT_CF32);               // cf32 [N] -i/2 * W_2N^k, the untangle twiddles
        words = tail() + at;
    }
};

#undef FEAT_LDS_FN
