/*
 * sir_hip.h -- C ABI of the MI355X-native speech-intent hot path (libsir_hip.so).
 *
 * The reference (avi2924/Speech-Intent-Recognizer) is pure Python on torch/torchaudio and has
 * no FFI of its own; its boundary for this path is the Python surface listed below.  Each entry
 * point here names the reference call it replaces (file:line under /root/reference).  The Python
 * host layer (speech-intent-recognizer_amd/) binds these with ctypes and keeps the reference's
 * signatures; INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions: plain C, no torch types.  Unless stated, every pointer is a DEVICE pointer owned by
 * the caller; `stream` is a hipStream_t passed as void*.  All calls are asynchronous on `stream`,
 * allocate nothing, and return 0 on success or a negative SIR_E* code (never throw);
 * sir_last_error() gives the message of the last failure on the calling thread.
 */
#ifndef SIR_HIP_H
#define SIR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIR_ABI_VERSION 1

#define SIR_OK 0
#define SIR_EINVAL (-1)   /* bad argument (shape, alignment, NULL) */
#define SIR_ENOMEM (-2)   /* workspace too small / hipMalloc failed */
#define SIR_EHIP (-3)     /* HIP runtime error */
#define SIR_EUNSUPPORTED (-4)
#define SIR_ETIMEOUT (-5) /* a GRU recurrence kernel gave up waiting for a peer workgroup: results invalid */

#define SIR_WAVE_F32 0
#define SIR_WAVE_I16 1    /* PCM16; dequantised as s / 32768 (torchaudio.load convention) */

typedef struct sir_handle sir_handle;

/* Feature-extractor configuration.
 * Replaces AudioFeatureExtractor.__init__ (scripts/precompute_features.py:21-36), i.e.
 * torchaudio MelSpectrogram(sample_rate, n_fft, hop_length, n_mels) + AmplitudeToDB() with their
 * defaults: win_length = n_fft (sir_create_ex takes another), periodic Hann, power 2, center + reflect pad, HTK mel,
 * norm None, f_min 0, f_max sample_rate/2, 10*log10(max(x,1e-10)).
 * `window` / `mel_fb` are optional HOST arrays (win_length floats; [n_fft/2+1][n_mels] dense, row-major)
 * so that the host can hand over torch's own float32 tables bit for bit; NULL = computed in double
 * here and rounded to float.
 * Supported front-ends: n_fft in {256, 512, 1024}, n_fft/16 <= hop_length <= n_fft (any integer), 1 <= win_length <= n_fft;
 * anything else is SIR_EUNSUPPORTED, and so is a caller's mel_fb whose taps do not fit the general kernel's LDS beside its other
 * buffers (about 3000 taps at n_fft 1024; the built-in bank has about 1000).  n_fft 1024 / hop 512 / win_length 1024 runs the specialised one-launch kernel
 * (feat_utt_kernel), every other one the general launch pair (DESIGN.md section 4 "Other front-ends"). */
typedef struct sir_feature_config {
    int sample_rate;   /* 16000 */
    int n_fft;         /* 1024; 256 and 512 are built too */
    int hop_length;    /* 512; any n_fft/16 .. n_fft */
    int n_mels;        /* 64 (<= 64) */
    float f_min;       /* 0 */
    float f_max;       /* sample_rate/2 */
    const float* window;
    const float* mel_fb;
} sir_feature_config;

/* Optional fused augmentation (scripts/augment.py:6-28 time_shift, :82-96 add_noise on the
 * waveform; scripts/dataset.py:160-176 SpecAugment masks on the features).  Any pointer may be
 * NULL (= that augmentation off).  All arrays are DEVICE arrays of length batch. */
typedef struct sir_augment {
    const int32_t* shift;        /* samples; >0 delays (zero fill on the left), <0 advances */
    const float* noise_sigma;    /* N(0, sigma^2) added per sample, counter-based RNG */
    uint64_t noise_seed;
    const int32_t* time_mask;    /* [batch][2] = {start frame, width}, width 0 = none */
    const int32_t* freq_mask;    /* [batch][2] = {start mel,   width} */
} sir_augment;

int sir_abi_version(void);
const char* sir_last_error(void);

/* Create / destroy a handle.  Uploads window, twiddles and the sparse mel filterbank to the
 * current HIP device (the only allocating calls).  Host-synchronous. */
int sir_create(const sir_feature_config* cfg, sir_handle** out);
/* sir_create with torch.stft's win_length: the window of win_length samples (cfg->window holds win_length floats, NULL = periodic
 * Hann of win_length computed in double) is centred in the frame of n_fft samples, (n_fft - win_length) / 2 zeros on its left.
 * win_length == 0 means n_fft; sir_create(cfg, out) is sir_create_ex(cfg, 0, out). */
int sir_create_ex(const sir_feature_config* cfg, int win_length, sir_handle** out);
int sir_destroy(sir_handle* h);

/* ---- waveform front-end --------------------------------------------
 * sir_mix_to_mono replaces `waveform = torch.mean(waveform, dim=0, keepdim=True)` after
 *   torchaudio.load (scripts/precompute_features.py:47-51, scripts/dataset.py:126-130,
 *   scripts/test_model.py:62-66) for a batch of decoded clips.
 *   pcm   : [batch][clip_stride] INTERLEAVED samples (frame-major, `channels` per frame), i16 or f32
 *           (dtype = SIR_WAVE_*); i16 is dequantised as s / 32768 first, as torchaudio.load does
 *   frames: device int32[batch] (NULL = all max_frames); out rows are zero beyond frames[b]
 *   out   : [batch][out_stride] f32 mono
 * sir_resample replaces `torchaudio.transforms.Resample(sr, 16000)(waveform)`
 *   (precompute_features.py:54-56, dataset.py:132-135, test_model.py:68-72): sinc_interp_hann,
 *   lowpass_filter_width 6, rolloff 0.99, output length ceil(new * length / orig) per clip.
 *   wave/lengths as in sir_features_fwd; out: [batch][out_stride] f32, zero beyond the clip's output
 *   length (clamped to max_out_len); out_lengths: optional device int32[batch].
 *   The first call for a rate pair builds the filter table on the host and uploads it (host-synchronous,
 *   two small hipMallocs owned by the handle); later calls only launch.
 *   lengths[b] above max_len is read as max_len; a NEGATIVE lengths[b] is an empty clip (zero row, out_lengths[b] = 0),
 *   as a negative frames[b] is for sir_mix_to_mono.  Neither kernel reads a sample at or behind a clip's length.
 * sir_resample_out_len: host helper, ceil(new * length / orig) with gcd-reduced rates; -1 on bad input (negative length,
 *   non-positive rate) and -1 when the value does not fit an int (2147483647 samples at 16000 -> 48000).
 * Tested against a direct float64 evaluation (tests/frontend_edge_ref.py) for sixteen rate pairs -- 44100 / 48000 / 16000 /
 *   22050 -> 8000, 11025 / 12000 / 32000 / 96000 / 22050 / 44100 -> 16000, 16000 -> 22050 / 48000 / 44100, 8000 -> 48000,
 *   44100 <-> 48000 -- at every tap of every phase and at the block and clip edges (tests/test_frontend_edge_gpu.py). */
int sir_mix_to_mono(sir_handle* h, const void* pcm, int dtype, int channels, int64_t clip_stride,
                    const int32_t* frames, int batch, int max_frames, float* out, int64_t out_stride,
                    void* stream);
int sir_resample_out_len(int length, int orig_freq, int new_freq);
int sir_resample(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride,
                 const int32_t* lengths, int batch, int max_len, int orig_freq, int new_freq, float* out,
                 int64_t out_stride, int max_out_len, int32_t* out_lengths, void* stream);

/* ---- waveform perturbation: pitch and tempo ---------------------------------
 * sir_wave_perturb replaces, for a whole batch, the two sox effects of scripts/augment.py:30-80 -- pitch_shift (`pitch c`
 * then `rate sr`) and speed_change (`tempo f` then `rate sr`) -- applied per utterance after the time shift, in the
 * reference's order (augment.py:119-133): shift, pitch, speed.  Noise and SpecAugment stay in sir_features_fwd.
 * Tempo is WSOLA as sox 14.4's `tempo` (default profile, linear search; segment / search / overlap from
 * h->cfg.sample_rate); pitch is tempo 1/d (d = 2^(c/1200)) resampled back to the clip's length at fractional positions
 * with sir_resample's windowed-sinc filter, not sox's `rate` filter.  No sample-level parity with sox is claimed.
 *   wave       : [batch][wave_stride] f32 or i16 (wave_dtype; i16 dequantised as s / 32768), row length lengths[b]
 *   shift      : optional device int32[batch], samples, as sir_augment.shift (NULL = none)
 *   pitch_cents: optional device f32[batch] in [-200, 200]; 0 = not drawn (NULL = none)
 *   tempo      : optional device f32[batch] in [0.5, 2] (> 1 faster and shorter); 1 = not drawn (NULL = none)
 *                A value outside its range zeroes that row (length 0) and is reported by sir_check_status (SIR_EINVAL).
 *   out        : [batch][out_stride] f32, zero beyond each row's output length
 *   out_lengths: optional device int32[batch] = min(sir_perturb_out_len(lengths[b], tempo[b]), max_out_len)
 *   offsets_out: optional test hook (NULL in production): int32 [batch][2][max_segments], the chosen WSOLA offset of each
 *                segment of the pitch pass (index 0) and the speed pass (index 1), -1 where unused
 *   workspace  : sir_perturb_workspace_bytes(batch, max_len) bytes, 256-byte aligned (may be NULL without pitch_cents)
 * sir_perturb_out_len: host helper, int(length / tempo + 0.5) in double (-1 on bad input). */
int sir_perturb_out_len(int length, float tempo);
size_t sir_perturb_workspace_bytes(const sir_handle* h, int batch, int max_len);
int sir_wave_perturb(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride, const int32_t* lengths, int batch,
                     int max_len, const int32_t* shift, const float* pitch_cents, const float* tempo, float* out,
                     int64_t out_stride, int max_out_len, int32_t* out_lengths, int32_t* offsets_out, int max_segments,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- room reverberation and background noise at a chosen SNR ----------------
 * sir_wave_reverb_mix: per row, with L = lengths[b] clamped to [0, max_len] and x the row's samples (i16 dequantised as
 * s / 32768), after sir_wave_perturb and ahead of sir_features_fwd:
 *   reverb  y[n] = sum_{k < min(K, n + 1)} x[n - k] h_r[k] for n in [0, L), r = rir_index[b], K = rir_lengths[r]: the head
 *           of the convolution with the room impulse response as given (no gain compensation; the tail beyond L is
 *           dropped, so lengths do not change).  r = -1: y = x bit for bit.  1 <= K <= max_rir_len <= 8192.
 *   noise   out[n] = y[n] + g v[(o + n) mod M], v = row noise_index[b] of the noise bank, M = noise_lengths[v] >= 1, o =
 *           noise_offset[b], g = sqrt(P_y / (P_v 10^(snr_db[b] / 10))), P_y = mean of y^2 over [0, L), P_v = mean square of
 *           the L noise samples used (with wrapping); g = 0 when P_y or P_v is 0.  v = -1: out = y bit for bit.
 *   out[b] is zero on [L, max_len) and untouched from max_len on; it must not overlap wave.  Nothing behind lengths[b] in
 *   wave, nor behind a bank row's length, is read.  Reductions are ordered (no atomics): results are bit-reproducible and
 *   row b depends on row b alone.
 *   rir_bank / noise_bank: [n][stride] f32 with device int32 lengths[n]; rir_index / noise_index: device int32[batch], NULL
 *   = that effect off for every row (its bank arguments are then ignored); noise_offset / snr_db: device [batch], read
 *   only where noise_index >= 0.
 *   An index outside [-1, n), a bank length outside its range, a NaN / infinite snr_db or a gain that is not a finite
 *   float32 (a finite snr_db far below the usable range: g passes FLT_MAX near -770 dB at ordinary levels) zeroes that
 *   row, reports gain 0 and is reported by sir_check_status (SIR_EINVAL); the other rows are unaffected.  A gain that
 *   underflows to 0 (snr_db far above the range) is no error: out = y bit for bit, gain 0.  A finite g whose product
 *   g v overflows float32 is plain float32 arithmetic and is not guarded.  lengths == NULL means max_len for every row;
 *   batch <= 65535.  max_rir_len > 8192: SIR_EINVAL.
 *   workspace: sir_reverb_workspace_bytes(batch, max_len, max_rir_len) bytes, 256-byte aligned (SIR_ENOMEM otherwise);
 *   its first `batch` floats receive the gain g applied to each row (0 where no noise was added). */
size_t sir_reverb_workspace_bytes(const sir_handle* h, int batch, int max_len, int max_rir_len);
int sir_wave_reverb_mix(sir_handle* h,
        const void* wave, int wave_dtype, int64_t wave_stride, const int32_t* lengths, int batch, int max_len,
        const float* rir_bank, int64_t rir_stride, const int32_t* rir_lengths, int n_rir, int max_rir_len,
        const int32_t* rir_index,                       /* device int32[batch]; -1 = no reverb for that row; NULL = none */
        const float* noise_bank, int64_t noise_stride, const int32_t* noise_lengths, int n_noise,
        const int32_t* noise_index,                     /* device int32[batch]; -1 = none; NULL = none */
        const int32_t* noise_offset, const float* snr_db,  /* device [batch]; read only where noise_index >= 0 */
        float* out, int64_t out_stride, void* workspace, size_t workspace_bytes, void* stream);

/* ---- feature path --------------------------------------------------------------------------
 * sir_features_fwd replaces, for a whole batch in one launch pair,
 *   AudioFeatureExtractor.extract_features  scripts/precompute_features.py:59-73
 *     (truncate is done by the caller through `lengths`; mel power, dB, whole-utterance z-norm)
 *   FSCIntentDataset.extract_features       scripts/dataset.py:137-152  (same arithmetic)
 *   pad / trim to t_pad frames              scripts/dataset.py:109-113, scripts/train.py:58-62
 * wave   : [batch][wave_stride] samples, f32 or i16 (wave_dtype), only [0, lengths[b]) is read
 * lengths: device int32[batch]; a clip with length <= n_fft/2 yields an all-zero row (the reference
 *          fails in torch.stft's reflect pad and substitutes zeros, dataset.py:121-123,156-158)
 * out    : [batch][n_mels][t_pad] f32; frames >= 1 + length/hop are zero
 * db_out : optional (NULL = off) [batch][n_mels][t_pad] f32 copy of the un-normalised dB values
 *          (10*log10(max(mel,1e-10)), zero in the padding) -- the AmplitudeToDB output of
 *          precompute_features.py:67, exposed so that the mel/dB stage can be checked on its own
 * workspace: sir_features_workspace_bytes(batch, max_len) bytes, 16-byte aligned: 256 on a handle of the default front-end
 *          (statistics stay on chip), on any other handle the dB slab [batch][n_mels][1 + max_len/hop] of the launch pair (every
 *          frame of a clip counts in its statistics, also those beyond t_pad); a smaller one is SIR_ENOMEM.
 * On the default front-end clips of more than 160 frames need t_pad >= their frame count; the general path has no such rule. */
size_t sir_features_workspace_bytes(const sir_handle* h, int batch, int max_len);
int sir_features_fwd(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride,
                     const int32_t* lengths, int batch, int max_len, float* out, int t_pad,
                     float* db_out, void* workspace, size_t workspace_bytes, const sir_augment* aug,
                     void* stream);

/* sir_features_bwd: the gradient of sir_features_fwd's `out` with respect to the waveform -- the chain z-norm, dB, mel filterbank,
 * power spectrum, real FFT, Hann window, framing with reflect padding, time shift -- in one launch (feat_utt_bwd_kernel:
 * DESIGN.md "Gradients down to the waveform").  The reference has no such path; torch autograd through the same operations
 * is the arithmetic it restates.  Asynchronous on `stream`; allocates nothing, uses no atomics and no workspace; bit-reproducible,
 * and row b depends on nothing but row b.
 *   wave, wave_dtype, wave_stride, lengths, max_len, t_pad, aug: exactly what the matching sir_features_fwd call got (lengths
 *            are clamped to max_len; noise is regenerated from aug->noise_seed, so the spectra are the forward's)
 *   db     : [batch][n_mels][t_pad] f32, the db_out that forward call wrote (required)
 *   dout   : [batch][n_mels][t_pad] f32, d loss / d out; entries in frames beyond the clip and in the SpecAugment bands of `aug`
 *            are ignored (those outputs are the constant 0 -- their positions still count in the statistics)
 *   dwave  : [batch][dwave_stride] f32, dwave_stride >= max_len; row b receives d loss / d sample for samples [0, lengths[b])
 *            (for PCM16 with respect to the dequantised s / 32768) and exact zeros in [lengths[b], max_len); written, not
 *            accumulated; columns >= max_len are not touched.  A clip with length <= n_fft/2 gives a zero row.
 * The statistics run over all frames of a clip and db holds t_pad of them: 1 + max_len / hop > t_pad is SIR_EUNSUPPORTED (no
 * partial answer).  A filterbank (sir_feature_config.mel_fb) with an FFT bin under more than two filters is SIR_EUNSUPPORTED.
 * Departures from autograd: where the mel power is at or below the 1e-10 clamp the gradient is 0 (the forward's own test), and a
 * clip whose dB tile is constant (sigma == 0, e.g. digital silence) gets dD = (g - mean g) / 1e-5 with the sigma term dropped,
 * where torch returns NaN.  NULL pointers, a bad dtype, misaligned pointers and strides < max_len are SIR_EINVAL; every
 * argument is checked before anything is launched.  The waveform gradient is built for the default front-end only: on a handle
 * that is not n_fft 1024 / hop 512 / win_length 1024 the call is SIR_EUNSUPPORTED and writes nothing. */
int sir_features_bwd(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride,
                     const int32_t* lengths, int batch, int max_len,
                     const float* db, const float* dout, int t_pad, const sir_augment* aug,
                     float* dwave, int64_t dwave_stride, void* stream);

/* ---- batch assembly from an HBM-resident feature store -----------------------------------------
 * sir_gather_features replaces, for a whole batch in one launch, what the reference does per item in DataLoader worker
 * processes and then copies over PCIe: FSCIntentDataset.__getitem__ (scripts/dataset.py:78-115: cache lookup, SpecAugment,
 * pad / trim -- the store rows are already padded to t_pad) + collate_fn's torch.stack (scripts/train.py:49-70) +
 * mel.to(device) (scripts/train.py:86).  The split's cached features live in HBM once (sir_amd/feature_store.py: a few
 * hundred MB of the 288 GB); a step's batch is a gather by index.
 *   store     : [n_store][n_mels][t_pad] f32 (device), rows zero beyond each clip's frames
 *   index     : device int64[batch], each in [0, n_store) (an index outside yields a zero row and SIR_EINVAL at the next
 *               sir_check_status)
 *   time_mask / freq_mask : optional device int32[batch][2] = {start, width} bands to zero (scripts/dataset.py:160-176,
 *               drawn by the host as torchaudio's mask_along_axis does); NULL = none
 *   out       : [batch][n_mels][t_pad] f32 */
int sir_gather_features(sir_handle* h, const float* store, int64_t n_store, const int64_t* index, int batch,
                        int n_mels, int t_pad, const int32_t* time_mask, const int32_t* freq_mask, float* out,
                        void* stream);

/* sir_mix_features: mixup (Zhang et al. 2018) on an ASSEMBLED feature batch -- after each item's own SpecAugment bands, so
 * that it serves every data route (sir_gather_features, a DataLoader batch, sir_features_fwd).  Replaces the torch lines
 * `x = lam * x + (1 - lam) * x[perm]`; the reference has no mixup (its configs/config.yaml carries an unread `mixup_alpha`).
 *   x    : [batch][n_mels][t] f32, 16-byte aligned, t a multiple of 4 (else SIR_EINVAL)
 *   perm : device int64[batch], batch-local partner rows; an entry outside [0, batch) yields a zero row and SIR_EINVAL at
 *          the next sir_check_status
 *   lam  : device f32[batch]
 *   out  : [batch][n_mels][t] f32, must not alias x; out[b] = fmaf(lam[b], x[b], (1.0f - lam[b]) * x[perm[b]]) in fp32,
 *          and a row with lam[b] == 1.0f is a bit-exact copy of x[b] whatever its partner holds (select, not multiply) */
int sir_mix_features(sir_handle* h, const float* x, const int64_t* perm, const float* lam, int batch, int n_mels, int t,
                     float* out, void* stream);

/* sir_adv_step: one ascent / projection step of an L-infinity adversary (FGSM: Goodfellow et al. 2015; PGD: Madry et al. 2018) on
 * an ASSEMBLED feature batch, in one launch.  Replaces the torch lines `x + eps * dx.sign()` of sir_amd.explain.fgsm and the
 * `x = clamp(x + alpha * g.sign(), x0 - eps, x0 + eps)` of a PGD loop; the reference has neither (it never attacks its model).
 *   x0, x, g, out : [batch][n_mels][t] f32 (device); n_mels in [1, 64], any t >= 1
 *   active        : device int32[batch], 0 = leave that row alone; NULL = every row is active
 * Gradient step (g != NULL; x is the current iterate and may be x0 itself): with s = +1 where g > 0, -1 where g < 0, else 0 (a
 * NaN gradient gives 0; a select, not a multiply),
 *     out = fminf(fmaxf(x + s * alpha, x0 - eps), x0 + eps)
 * in fp32, every operation rounded on its own (nothing is contracted).  out may BE x (in place); it must not overlap x0 or g.
 * Random start (g == NULL; x must be NULL too, alpha is not read): U = the 24-bit uniform of the dropout mask's hash (hash of
 * start_seed and the element index (b * n_mels + m) * t + j, >> 40, * 2^-24), r = 2 U - 1 (exact),
 *     out = fminf(fmaxf(x0 + eps * r, x0 - eps), x0 + eps).
 * Left alone -- bit-exact copies of x0, -0.0 and NaN payloads included (a select between words, no arithmetic): every row with
 * active[b] == 0 and, with keep_zero_columns, every frame column j of row b whose n_mels values of x0 are all bit pattern 0.
 * Zero padding and SpecAugment time bands so stay what they were (sir_model_infer's pad-skip rule: a column of -0.0 is data).
 * NULL h / x0 / out / cfg, batch or t < 1, n_mels outside [1, 64], a negative or NaN eps (or alpha, on a gradient step), x
 * without g, g without x, a forbidden overlap and a pointer that is not 4-byte aligned are SIR_EINVAL; every argument is checked
 * before the launch and a refused call writes nothing.  No allocation, no workspace, no atomics, no status bit; row b depends
 * on row b alone.  16-byte accesses when t % 4 == 0 and all pointers are 16-byte aligned, element accesses otherwise. */
typedef struct sir_adv_config {
    float eps;                /* radius of the L-infinity ball around x0, >= 0 */
    float alpha;              /* step size, >= 0 (not read on a random-start call) */
    int   keep_zero_columns;  /* != 0: a frame column of x0 whose n_mels values are all +0.0 (bit pattern 0) is left as it is */
} sir_adv_config;
int sir_adv_step(sir_handle* h, const float* x0, const float* x, const float* g, const int32_t* active,
                 int batch, int n_mels, int t, const sir_adv_config* cfg, uint64_t start_seed,
                 float* out, void* stream);

/* ---- model path ----------------------------------------------------------------------------
 * Device pointers to the reference's parameters/buffers under their state_dict names
 * (models/models.py:10-39): index 0..2 = conv1..3 / bn1..3; GRU index = 2*layer + reverse. */
typedef struct sir_model_weights {
    const float* conv_w[3];      /* [32,1,3,3] [64,32,3,3] [128,64,3,3], no bias */
    const float* bn_w[3];
    const float* bn_b[3];
    const float* bn_mean[3];     /* running_mean */
    const float* bn_var[3];      /* running_var  */
    const float* gru_w_ih[4];    /* [768,1024] x2, [768,512] x2 ; gate order r,z,n */
    const float* gru_w_hh[4];    /* [768,256] */
    const float* gru_b_ih[4];    /* [768] */
    const float* gru_b_hh[4];    /* [768] */
    const float* attn_w;         /* [1,512] */
    const float* attn_b;         /* [1] */
    const float* fc_w;           /* [num_classes,512] */
    const float* fc_b;           /* [num_classes] */
    int num_classes;             /* <= 64 */
} sir_model_weights;

/* sir_model_infer replaces CNNAudioGRU.forward in eval() (models/models.py:41-68) followed by
 * torch.argmax(outputs, dim=1) (scripts/evaluate.py:82-83) / torch.max (scripts/train.py:149).
 * feats  : [batch][64][t_frames] f32 (8 <= t_frames <= 2055; 200 on the training path)
 * logits : [batch][num_classes] f32
 * argmax : int64[batch] or NULL
 * workspace: sir_model_workspace_bytes(batch, t_frames, 0) bytes, 256-byte aligned
 * Trailing frame columns whose 64 values are all exactly +0.0 (bit pattern 0) are treated as padding: conv1-3 and the
 * layer-0 input projection skip every position that sees only such columns, and the recurrence takes those positions'
 * values from an all-zero template utterance computed beside the batch.  Results are bit-identical to the full
 * computation; a tail of -0.0 (or any other non-zero bits) is computed in full.  The intermediate buffers listed by
 * sir_model_workspace_offsets hold valid values only for the computed positions: past them they are left unwritten. */
size_t sir_model_workspace_bytes(const sir_handle* h, int batch, int t_frames, int train);
/* Byte offsets of the buffers inside the inference workspace (S = t_frames / 8 GRU steps; n = B + 1: the batch and, at index B,
 * the all-zero template utterance of the pad skip), so that tests can check every stage against the oracle:
 *    0  a1     conv1 block output (pooled), NHWC           [n][32][T/2][32]
 *    1  a2     conv2 block output, NHWC                    [n][16][T/4][64]
 *    2  x0     conv3 block output = GRU layer 0 input      [n][S][1024] (feature = c*8+h, models.py:55-57)
 *    3  gi     input projection of the running layer       [n*S][1536]
 *    4  y0     GRU layer 0 output                          [B][S][512]
 *    5  y1     GRU layer 1 output                          [B][S][512]
 *    6  ctx    attention-pooled context                    [B][512]
 *    7  pad    the int tables of the pad skip / of a ragged call: sir_model_infer_table_offsets
 *    8  xz     the template utterance's all-zero features  [64][T]
 *    9  bn     folded BatchNorm: scale, shift              [2][224] (bn1 | bn2 | bn3 at channels 0, 32, 96)
 *   10  wht    W_hh as the recurrence's resident fragments, (layer, direction)
 *   11  xs     16-bit planes of the input-projection GEMM's A operand   [2][n*S][1024]
 *   12  ws     16-bit planes of W_ih (both layers, both directions)
 *   13  wcb    16-bit planes of the conv2 / conv3 weights
 *   14, 15     reserved (no bytes)
 * Slots 0..3 and 11 hold values only for the computed positions (see above; a ragged call: the positions inside each utterance's
 * own width); slots 4..6 are written in full by a padded call, and for t < frames[b] / 8 by a ragged one.  Slots 9, 10, 12 and 13
 * are the prepared weights (sir_model_set_weights_version).  `train` is ignored: the training workspace has a list of its own,
 * sir_model_train_workspace_offsets.  Needs no device and ignores h.  Returns the number of buffers (16), or SIR_EINVAL for an
 * unsupported shape. */
int sir_model_workspace_offsets(const sir_handle* h, int batch, int t_frames, int train,
                                size_t* offsets, int n);
/* The int tables inside slot 7 of the list above.  Writes up to n values: the offsets, in ints from the slot's start, of
 *   0 e0         [B]      1 + last frame column with any bit set (a ragged call: frames[b], or 0 where that is outside [8, T])
 *   1 d1         [B + 1]  conv1 columns computed per utterance (the template utterance last)
 *   2 d3         [B + 1]  GRU steps of each utterance that see data (a ragged call: its own steps, frames[b] / 8)
 *   3 rows       the layer-0 projection's row list: the count, then that many rows u * S + s, ascending
 *   4 tab2       conv2's task list: {count, unused}, then two words per task
 *   5 tab3       conv3's task list, likewise
 *   6 record     {rows read, tile height chosen} of the latest row-list input projection
 *   7 nonfinite  [B]      1 where an utterance's features hold a NaN or an infinity
 * then (8) the slot's size in ints and (9) the slot's index in sir_model_workspace_offsets.  Needs no device and ignores h.
 * Returns the number of values (10), or SIR_EINVAL for an unsupported shape. */
int sir_model_infer_table_offsets(const sir_handle* h, int batch, int t_frames, size_t* offsets, int n);
/* Optional: tell the library which version of the weights the next sir_model_infer calls will see.  The
 * derived weight layouts (bf16x3 planes, folded BatchNorm, ...) live in the caller's workspace; when the
 * version is non-zero and unchanged since the previous call with the same workspace and shape, they are
 * reused instead of rebuilt (~40 us per call).  0 (the default) = always rebuild. */
int sir_model_set_weights_version(sir_handle* h, uint64_t version);
/* Batch regimes (256 CUs): the GRU recurrences hold half the chip at batch 256 and all of it at 512; beyond that they are oversubscribed and rest
 * on in-order dispatch.  Tested against the oracle up to batch 1041 (tests/test_large_batch_gpu.py).  Token range: the training step is
 * tested against the float64 oracle from 1 token (batch 1 of 8 frames; token count = batch * (t_frames / 8)) to 10240 tokens (batch 405 of
 * 200 frames, batch 40 of 2048), dense and ragged inference at every length from 8 to 17 frames, 23, 24 and 31
 * (tests/test_token_range_gpu.py).  One step runs at batch 2048 of 256 frames (65536 tokens), the first shape at which the conv plan
 * picks a fallback kernel by itself -- conv2's nine-tap weight gradient: that gradient is checked against a float64 contraction of the
 * step's own operands, loss and all 29 gradients are finite and no recurrence times out (tests/test_conv_fallback_gpu.py).  Untested
 * against the oracle of the whole step: token counts above 10240 in training, and batches above 1100.
 * Sequence regimes: 8 <= t_frames <= 2055 on every model entry point, inference and training alike (a shape outside it, or a batch above
 * 65535, is SIR_EINVAL; sir_model_workspace_bytes returns 0), with ONE exception, in the training backward: the conv2 / conv3 weight
 * gradient is SIR_EUNSUPPORTED when batch * t_frames >= 524288 with t_frames >= 258 (conv2; e.g. batch 256 of 2048 frames, 512 of 1024);
 * for conv3 from batch * t_frames >= 1048576 with t_frames >= 260.  Beyond those products a stage's dz no longer fits the 32-bit byte
 * offsets of the Winograd weight-gradient kernel, and the nine-tap kernel that takes over holds one map row of at most 128 (conv2) / 64
 * (conv3) columns.  sir_model_train_bwd, _part (either half), _cfg and _x refuse such a call before anything is launched and write
 * nothing; with that conv weight's gradient pointer NULL (frozen) the call runs.  The forward and inference have no such limit
 * (tests/test_conv_fallback_gpu.py).  The GRU runs S = t_frames / 8 steps and the attention kernels hold one
 * score per step in LDS arrays of 256, which is what limits the range: 2055 frames are 256 steps -- 20 s at a 10 ms hop, 65 s at the default
 * 32 ms one.  The step field of a recurrence exchange tag (9 bits, step + 1) ends there as well.  Tested against the oracle up to 2055 frames
 * (tests/test_long_sequence_gpu.py), at batches up to 17 in inference and up to 8 in training.
 *
 * Operand range and non-finite values (sir_model_infer, sir_model_infer_ragged, sir_model_train_fwd*, sir_model_train_bwd*;
 * tests/test_operand_range_gpu.py).  The contractions split every fp32 operand into two fp16 planes, and the convolution kernels
 * apply ReLU and max-pool as fmaxf; neither carries a NaN.  What the callers get instead:
 *   features   inference: a NaN or an infinity anywhere in utterance b (ragged: in its frames[b] columns) makes ALL of row b of
 *              logits NaN (argmax 0); every other row is bit-identical to what it is without that value.  No status bit.
 *              training forward with live bn1 statistics: a non-finite feature anywhere makes EVERY row of logits NaN (batch
 *              statistics carry it into all of them), hence a NaN loss, NaN dlogits and NaN fc gradients -- isfinite(loss) and the
 *              total norm of sir_grad_norm both see it.  No status bit.  The test is on the fp32 sum of the squared features, so a
 *              finite feature beyond ~1.8e19 in magnitude (its square overflows fp32) counts as non-finite.
 *              training forward with bn_frozen[0] (a frozen-statistics fine-tune, sir_amd.explain): the features are NOT looked at;
 *              a non-finite feature gives finite, meaningless logits and loss there.
 *   conv2 / conv3 weights   a transformed weight U = G g G^T with |U| >= 32, or not finite: status bit 3 (SIR_EINVAL at the next
 *              sir_check_status); the outputs are computed from the clamped value.  Below 32 the planes are exact.  That is the fp16
 *              planes' limit: a stage on its shape fallback (bf16x3 planes, fp32's exponent range) raises no bit for a finite |U| >= 32
 *              and computes from the exact value -- at U = 40 logits and all 29 gradients hold their float64 bounds
 *              (tests/test_conv_fallback_gpu.py); which kernels a shape gets is the library's choice, so keep |U| < 32.
 *   GRU weight_ih / weight_hh   an element beyond +-65504 or not finite: status bit 11 (SIR_EINVAL); outputs from the clamped value.
 *   attention, fc   used in fp32 behind the last ReLU: a non-finite value comes out where torch has it (a NaN in fc.weight[j][.]
 *              makes exactly logit column j NaN).
 *   conv1 weights, BatchNorm weight / bias / running statistics   sit in front of an fmaxf ReLU / max-pool, which drops a NaN (the
 *              logits come out finite): a non-finite value raises status bit 13 (SIR_EINVAL) in the kernels that fold them --
 *              inference and frozen blocks: weight, bias and both running statistics; a block on batch statistics: weight and
 *              bias (its running statistics are written, not used); conv1's weights with bn1 either way.
 *   GRU biases   not tested, unspecified.
 *   activations   the training forward raises status bit 12 (SIR_EINVAL) when the conv2 block writes an output >= 256 or the conv3
 *              block one >= 512: beyond these the backward's single-accumulator WEIGHT-gradient contractions (the conv3 weight
 *              gradient, the GRU layer-0 weight-gradient GEMM) clamp or saturate that operand.  Up to there gradients are tested
 *              against float64.  The forward does not know what the backward will be asked for, so the bit is raised whatever
 *              follows: logits, loss and the input gradient (sir_model_train_bwd_x) do not read these operands and stay valid.
 *              The conv1 block output feeds the conv2 weight gradient under the same limit of 256 and is NOT checked.
 *              Bit 12 is raised on the shape fallbacks too, whatever the conv plan: with conv3's weight gradient on the nine-tap bf16x6
 *              kernel a conv2 block output of 300 leaves all 29 gradients inside their float64 bounds (conv3.weight 1.2e-4 * rms,
 *              against 0.33 * rms from the clamped value on the Winograd kernel), and the bit is then a false alarm for that call.
 *   dlogits    sir_model_train_bwd* accepts any finite magnitude: one small kernel picks the backward's internal power-of-two scale
 *              from max |dlogits| (workspace slot 39), so gradients are as accurate at (softmax - onehot) ~ 2^-24 as at ~ 1, and a
 *              scaled loss (dlogits x 2^16) does not saturate.  A NaN / infinite dlogits makes the fc gradients (fp32, straight from
 *              dlogits) non-finite, and with them the total norm of sir_grad_norm; the other gradients pass clamping splits and
 *              are unspecified. */
int sir_model_infer(sir_handle* h, const sir_model_weights* w, const float* feats, int batch,
                    int t_frames, float* logits, int64_t* argmax, void* workspace,
                    size_t workspace_bytes, void* stream);
/* sir_model_infer_ragged replaces the un-padded scoring of scripts/test_tts_samples.py:83-96 -- each file fed at its own
 * length as [1, 1, 64, T] through model(features), softmax / torch.max / topk left to the caller -- for a whole batch of
 * mixed-length clips in one call.
 * feats  : [batch][64][t_frames] f32; row b holds frames[b] feature columns, the columns behind them are never read as data
 * frames : int32[batch] in DEVICE memory, 8 <= frames[b] <= t_frames
 * logits : row b = CNNAudioGRU.forward(feats[b:b+1, :, :frames[b]]) in eval(): widths W1 = frames / 2, W2 = W1 / 2,
 *          S_b = W2 / 2; every convolution takes its right edge at the utterance's own width (the odd column MaxPool2d(2)
 *          drops is dropped), the GRU runs S_b steps (the reverse direction starts at S_b - 1 from h = 0) and the attention
 *          softmax runs over t < S_b.  A clip's logits do not depend on its position in the batch or on its neighbours.
 * argmax, workspace (sir_model_workspace_bytes(h, batch, t_frames, 0) bytes, the size sir_model_infer asks for), stream: as
 * sir_model_infer; the prepared weights are shared with it (same workspace and shape: nothing is rebuilt, whatever `frames` holds).
 * A frames[b] outside [8, t_frames] makes row b of logits NaN (argmax 0) and raises the handle's status word: SIR_EINVAL at the
 * next sir_check_status.  The other rows are unaffected.  Intermediate buffers are written only inside each utterance's widths. */
int sir_model_infer_ragged(sir_handle* h, const sir_model_weights* w, const float* feats,
                           const int32_t* frames, int batch, int t_frames, float* logits,
                           int64_t* argmax, void* workspace, size_t workspace_bytes, void* stream);
/* sir_model_embed: the forward of sir_model_infer (frames == NULL) or of sir_model_infer_ragged (frames: DEVICE int32[batch]),
 * returning the utterance embedding: the attention-pooled context (models/models.py:63-66), 512 floats per utterance, raw and
 * un-normalised.  Workspace size, prepared-weight reuse, shape limits and the status word are those of the two calls.
 * emb    : [batch][512] f32, 16-byte aligned, required.  For every row to which sir_model_infer* gives finite logits it is
 *          bit-identical to workspace slot 6 (sir_model_workspace_offsets); it is all-NaN for every row those calls make NaN: a
 *          non-finite feature in the utterance, or a ragged length outside [8, t_frames].  One small kernel behind the head
 *          (copy + the NaN rule); the forward kernels, their outputs and the workspace contents are exactly sir_model_infer*'s.
 * logits : [batch][num_classes] or NULL.  When given, logits (and argmax, optional, needs logits) are bit-identical to
 *          sir_model_infer / sir_model_infer_ragged; with logits == NULL the classifier is not run. */
int sir_model_embed(sir_handle* h, const sir_model_weights* w, const float* feats, const int32_t* frames /* NULL: padded */,
                    int batch, int t_frames, float* emb, float* logits, int64_t* argmax, void* workspace,
                    size_t workspace_bytes, void* stream);
/* ---- utterance segmentation of long recordings --------------------------------
 * sir_vad_segment replaces, for a whole batch of recordings resident in HBM, the energy detector of the continuous-audio
 * recogniser: MicrophoneListener._calculate_energy / _is_speech (scripts/testing.py:38-47) and the state machine of
 * MicrophoneListener.listen (:63-133).  sir_vad_gather cuts the found utterances out as the float rows IntentRecognizer.predict
 * (:222-266) is handed (`audio_float`, :118-119), trimmed in samples as :231-232 trims in frames.
 * For recording r of lengths[r] samples and chunk size c: n_chunks = ceil(lengths[r] / c); a trailing partial chunk is judged on
 * its own samples (the reference's stream never delivers one).
 *   energy  : e_k = mean |x| over the chunk's samples (:38-42).  i16: the integer sum S of |s| is exact and
 *             e_k = (float)((double)S / (count * 32768.0)), the correctly rounded mean.  f32: an ordered, atomic-free fp32
 *             reduction (at most chunk_size / 64 + 6 additions on any path, then one division): bit-reproducible run to run.
 *             speech_k = e_k > threshold, strict, in float (:44-47); a NaN energy is silence.
 *   segments: with P = prior_chunks, n_stop = silence_chunks -- a segment TRIGGERS at speech chunk i if no speech chunk precedes
 *             it or the previous one lies more than n_stop back (:85-92); it ENDS at chunk j if speech_{j - n_stop} holds and
 *             the n_stop chunks after it are silent (:104-115; n_stop == 0: every speech chunk is its own segment).  The k-th
 *             trigger pairs with the k-th end; the segment's first chunk is max(0, i - P + 1) for P >= 1 (the prior buffer of
 *             :79-82 already holds chunk i) and i for P == 0; its samples are [first * c, min((j + 1) * c, length)).
 *             As the reference: the prior buffer is not cleared between utterances, so a segment may start up to P - 1 chunks
 *             inside the previous one, and the trailing n_stop silent chunks belong to the segment.
 *             Unlike the reference: (1) it appends the trigger chunk twice (from the prior buffer and at :96); here a segment is
 *             a contiguous sample range and that chunk appears once.  (2) it drops an utterance still open when the stream
 *             stops; flush_tail != 0 emits it, ending at `length`; flush_tail == 0 drops it.
 *   wave, wave_dtype, wave_stride, lengths, max_len: as sir_features_fwd (lengths are clamped to [0, max_len])
 *   energy_out: optional test hook (NULL in production): f32 [n_rec][max_chunks], max_chunks = ceil(max_len / chunk_size), zero
 *               behind a recording's own chunks.  Without it only the packed speech flags are written (into the workspace).
 *   seg_count : int32 [n_rec], the TRUE number of segments of each recording
 *   seg_table : int32 [seg_cap][3] = {recording, start sample, end sample}, recording-major, then by time; rows at or beyond
 *               min(total, seg_cap) are left unwritten (may be NULL when seg_cap == 0)
 *   total     : int32 [1], the true total.  It stays on the device; a total above seg_cap is not an error of the call -- the host
 *               sees it in `total`, grows the table and calls again.  (The total must stay below 2^31.)
 *   workspace : sir_vad_workspace_bytes(h, n_rec, max_len, chunk_size) bytes, 16-byte aligned (too small: SIR_ENOMEM)
 * Nothing allocates, nothing synchronises; the numbering uses prefix scans, no atomics: the table order is exact.
 * sir_vad_gather: row s < min(total, seg_cap) of `out` ([seg_cap][out_stride] f32) = the segment's samples (i16 dequantised as
 *   s / 32768), cut at max_clip_len, zero behind its length up to max_clip_len; out_lengths[s] = min(end - start, max_clip_len).
 *   Rows at or beyond min(total, seg_cap) get out_lengths = 0 and are not otherwise written.  A table row with a recording
 *   outside [0, n_rec) or a range outside 0 <= start <= end <= wave_stride yields a zero row of length 0 and raises the handle's
 *   status word (bit 128): SIR_EINVAL at the next sir_check_status.  The other rows are unaffected.
 * sir_vad_stop_chunks: host helper, the smallest n with n * (chunk_size / sample_rate) >= silence_limit evaluated in double as
 *   the listener's own test (:110-111); 16 at its defaults.  -1 on bad input (a rate or chunk size <= 0, a limit that is
 *   negative, NaN or infinite).  prior_chunks is int(prior_recording * sample_rate / chunk_size) (:63), 7 at the defaults. */
typedef struct sir_vad_config {
    int   chunk_size;      /* 1024; in [64, 4096], a multiple of 64 (else SIR_EINVAL) */
    float threshold;       /* 0.01; NaN or < 0: SIR_EINVAL */
    int   silence_chunks;  /* >= 0 */
    int   prior_chunks;    /* >= 0 */
    int   flush_tail;      /* != 0: emit an utterance still open at the end of the recording */
} sir_vad_config;
int sir_vad_stop_chunks(int sample_rate, int chunk_size, double silence_limit);
size_t sir_vad_workspace_bytes(const sir_handle* h, int n_rec, int max_len, int chunk_size);
int sir_vad_segment(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride, const int32_t* lengths, int n_rec,
                    int max_len, const sir_vad_config* cfg, float* energy_out, int32_t* seg_count, int32_t* seg_table, int seg_cap,
                    int32_t* total, void* workspace, size_t workspace_bytes, void* stream);
int sir_vad_gather(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride, int n_rec, const int32_t* seg_table,
                   const int32_t* total, int seg_cap, float* out, int64_t out_stride, int max_clip_len, int32_t* out_lengths,
                   void* stream);

/* ---- live streams: segment audio that arrives piece by piece -------------------
 * The same detector with carried state: S independent streams, each fed a few samples per call, the way MicrophoneListener.listen
 * (scripts/testing.py:63-133) reads its microphone 1024 samples at a time.  All state lives in ONE caller-owned device buffer
 * (`state`, sir_stream_state_bytes bytes, 256-byte aligned): per stream the counters of the state machine and a ring of
 * R = ring_chunks chunks of samples, plus the flag bytes of the latest push.  Nothing allocates, nothing synchronises, no atomics on
 * the numbering path: every output is bit-reproducible, and the table a stream produces does not depend on how its samples were
 * cut into pushes.  With c = vad.chunk_size, P = vad.prior_chunks, n_stop = vad.silence_chunks, M = max_utt_chunks:
 *   state per stream: n samples received and j chunks judged since its last reset, recording, silence, first.  Sample positions
 *     in the table count from the stream's last reset (int64).  Chunk k lives at ring offset (k mod R) * c, always contiguous.
 *   sir_stream_reset: zeroes the state of the streams with mask[s] != 0 (mask == NULL: all).  Must run once before the first push.
 *   sir_stream_push : appends m_s = clamp(in_lengths[s], 0, min(in_width, max_in)) samples of row s of `in` ([S][in_stride],
 *     wave_dtype) to stream s, then judges, in order, every complete chunk not judged yet.  m_s == 0 (and no close): untouched.
 *     chunk i: speech = e_i > threshold, e_i exactly sir_vad_segment's energy (same integer sum for i16, same fp32 reduction order
 *       for f32, however many pushes assembled the chunk).
 *       1. not recording and speech: recording starts, silence = 0, first = max(0, i - P + 1) (P == 0: first = i).
 *       2. recording: silence = speech ? 0 : silence + 1; if silence >= n_stop the row {s, first * c, min((i + 1) * c, n), 0} is
 *          emitted and recording stops; else if i - first + 1 >= M the same row is emitted with flag bit 0 (1, forced) and
 *          recording stops: the next speech chunk triggers a new utterance, whose `first` may lie inside the previous one as the
 *          reference's uncleared prior buffer allows.
 *     close[s] != 0 (close == NULL: none), after the above: a trailing partial chunk is judged on its own samples as the batch
 *       form does; an utterance still open is emitted ending at n with flag bit 1 (2, flushed) if vad.flush_tail != 0; the
 *       stream's state returns to zero (the slot can take a new caller); its ring stays readable until the next push.
 *     energy_out: optional test hook (NULL in production), f32 [S][K], K = ceil(max_in / c) + 1: the energies of the chunks this
 *       push judged, in order, zero behind them.
 *     seg_table : int64 [seg_cap][4] = {stream, start sample, end sample, flags}, stream-major then by time, rows [0, total);
 *       seg_cap < sir_stream_max_rows(cfg) is SIR_EINVAL before anything is launched (the state has not moved: a push never
 *       loses a row).  total: int32 [1], stays on the device.
 *   sir_stream_gather: as sir_vad_gather, but position p of stream s is read at ring offset p mod (R * c) and the stream comes
 *     from column 0 of the row.  It must be queued before the next push on the same state: R >= sir_stream_min_ring_chunks keeps
 *     every row of the latest push intact until then.  A row with a stream outside [0, S) or a range that is not
 *     0 <= start <= end <= start + R * c yields a zero row of length 0 and raises the handle's status word (bit 1024): SIR_EINVAL
 *     at the next sir_check_status; the other rows are unaffected.
 * SIR_EINVAL: NULL pointers, a bad wave_dtype, a vad part sir_vad_segment would refuse, n_streams outside [1, 65535], max_in
 * outside [1, 2^24], M <= P or M > 2^20, R below the minimum or above 2^21 (the upper bounds keep every byte count and row count
 * far from overflow; a sir_stream_max_rows above 2^31 - 1 is refused too), a state that is not 256-byte aligned, in_width outside
 * [1, max_in] or above in_stride.  sir_stream_state_bytes returns 0 for a config the calls would refuse.  state_bytes too small:
 * SIR_ENOMEM.  These launches carry no profile ids (sir_profile_kernel_count is unchanged). */
#define SIR_STREAM_FORCED  1   /* flags column: the utterance reached max_utt_chunks and was ended there */
#define SIR_STREAM_FLUSHED 2   /* flags column: the utterance was still open when its stream was closed */
typedef struct sir_stream_config {
    sir_vad_config vad;      /* chunk_size, threshold, silence_chunks, prior_chunks, flush_tail: same meaning and same checks */
    int n_streams;           /* S, 1 .. 65535 */
    int wave_dtype;          /* SIR_WAVE_I16 | SIR_WAVE_F32: dtype of the pushes and of the ring */
    int max_in;              /* most samples one push may bring per stream, >= 1 */
    int max_utt_chunks;      /* M > prior_chunks: an utterance that reaches M chunks is ended there (forced) */
    int ring_chunks;         /* R >= sir_stream_min_ring_chunks(cfg) */
} sir_stream_config;
int sir_stream_min_ring_chunks(const sir_stream_config* cfg);   /* M + ceil(max_in / c) + 2; -1 on a bad config */
int sir_stream_max_rows(const sir_stream_config* cfg);          /* S * (ceil(max_in / c) + 2): the most rows one push can emit; -1 on a bad config */
size_t sir_stream_state_bytes(const sir_handle* h, const sir_stream_config* cfg);
int sir_stream_reset(sir_handle* h, void* state, size_t state_bytes, const sir_stream_config* cfg, const uint8_t* mask, void* stream);
int sir_stream_push(sir_handle* h, void* state, size_t state_bytes, const sir_stream_config* cfg, const void* in, int64_t in_stride,
                    int in_width, const int32_t* in_lengths, const uint8_t* close, float* energy_out, int64_t* seg_table, int seg_cap,
                    int32_t* total, void* stream);
int sir_stream_gather(sir_handle* h, const void* state, size_t state_bytes, const sir_stream_config* cfg, const int64_t* seg_table,
                      const int32_t* total, int seg_cap, float* out, int64_t out_stride, int max_clip_len, int32_t* out_lengths,
                      void* stream);

/* ---- live streams at the caller's rate and codec (DESIGN.md section 4 "Stream input") ----------------------------------
 * The stage in front of sir_stream_push for audio that does not arrive as PCM at the handle's rate: S independent streams of
 * G.711 bytes, int16 or float32 at in_rate, each decoded and rate-converted to float32 at out_rate push by push, with the filter
 * state carried in ONE caller-owned device buffer (`state`, sir_stream_input_state_bytes bytes, 256-byte aligned).  The
 * concatenation of a stream's outputs over its life is bit for bit what sir_resample returns for the whole decoded stream: it does
 * not depend on how the samples were cut into pushes.  Conventions are sir_stream_push's: asynchronous on `stream`, nothing
 * allocates in push (the first reset for a rate pair builds the filter table host-synchronously, as the first sir_resample does),
 * no atomics, stream s depends on stream s alone, every argument is checked before any launch, a refused call writes nothing and
 * leaves the state where it was, no profile ids.
 *   decoding : to a 16-bit linear value v, then x = v / 32768 (exact).  mu-law byte b: u = ~b & 0xFF, t = (((u & 0x0F) << 3) + 0x84)
 *     << ((u >> 4) & 7), v = (u & 0x80) ? 0x84 - t : t - 0x84.  A-law byte b: a = b ^ 0x55, e = (a >> 4) & 7, m = a & 0x0F,
 *     t = e ? ((m << 4) + 0x108) << (e - 1) : (m << 4) + 8, v = (a & 0x80) ? t : -t.  I16: s / 32768.  F32: as it is.
 *   filter   : sir_resample's table for (in_rate, out_rate) -- gcd-reduced orig and nw, width, chain length L, first[p], taps[p][l].
 *     Output j = q nw + p is the chain acc = fmaf(taps[p][l], x[q orig + first[p] - width + l], acc), l = 0 .. L - 1, from acc = 0,
 *     with x[i] = 0 for i < 0 and, once the stream is closed at n samples, for i >= n: resample_kernel's chain, tap for tap.
 *   emission : output j needs need(j) = q orig + first[p] - width + L samples.  E(n) = the largest J with need(j) <= n for all
 *     j < J.  A stream that has received n samples has emitted exactly the outputs j < E(n): a push that takes it from n0 to n1
 *     writes outputs E(n0) .. E(n1) - 1 to out[s][0 ..] and their count to out_lengths[s]; columns behind the count are not written.
 *     m_s = clamp(in_lengths[s], 0, min(in_width, max_in)); only [0, m_s) of row s of `in` ([S][in_stride], elements of in_dtype)
 *     is read.  m_s == 0 without close: the stream is untouched, out_lengths[s] = 0.
 *     close[s] != 0 (close == NULL: none), after the append: the outputs up to sir_resample_out_len(n1, in_rate, out_rate) are
 *     emitted with the zero tail, and the stream's counters return to zero (the slot can take a new caller from position 0).
 *     in_rate == out_rate: out is the decoded input, out_lengths[s] = m_s, nothing is held back.
 *   state    : per stream n and the emitted count (int64), and a ring of the most recent H = 2 (2 width + orig) decoded float32
 *     samples (sample i at ring offset i mod H); H = 0 when the rates are equal.  Never the stream.
 *   sir_stream_input_max_out: the most outputs one push can emit per stream, ceil(nw (max_in + 3 width + 2 orig) / orig) + 1
 *     (E(n) >= nw (n - 3 width - 2 orig) / orig and out_len(n + m) < nw (n + m) / orig + 1); max_in when the rates are equal.
 *     out_stride below it is SIR_EINVAL.  -1 on a bad config or when the value does not fit an int.
 *   sir_stream_input_reset: zeroes the counters of the streams with mask[s] != 0 (mask == NULL: all).  Must run once before the
 *     first push.
 * SIR_EINVAL: NULL pointers, a bad in_dtype, rates <= 0, n_streams outside [1, 65535], max_in outside [1, 2^24], in_width outside
 * [1, max_in] or above in_stride, a state that is not 256-byte aligned, out_stride below sir_stream_input_max_out, a max_out that
 * does not fit an int.  state_bytes too small: SIR_ENOMEM.  sir_stream_input_state_bytes returns 0 for a config the calls refuse.
 * SIR_WAVE_ULAW / SIR_WAVE_ALAW are accepted ONLY here: every other entry point keeps refusing them. */
#define SIR_WAVE_ULAW 2   /* G.711 mu-law, one byte per sample; accepted ONLY by sir_stream_input_* */
#define SIR_WAVE_ALAW 3   /* G.711 A-law, likewise */
typedef struct sir_stream_input_config {
    int n_streams;   /* S, 1 .. 65535 */
    int in_dtype;    /* SIR_WAVE_F32 | SIR_WAVE_I16 | SIR_WAVE_ULAW | SIR_WAVE_ALAW */
    int in_rate;     /* Hz, > 0 */
    int out_rate;    /* Hz, > 0; == in_rate is legal (decode / copy only) */
    int max_in;      /* most samples one push may bring per stream, 1 .. 2^24 */
} sir_stream_input_config;
int    sir_stream_input_max_out(const sir_stream_input_config* cfg);
size_t sir_stream_input_state_bytes(const sir_handle* h, const sir_stream_input_config* cfg);
int    sir_stream_input_reset(sir_handle* h, void* state, size_t state_bytes, const sir_stream_input_config* cfg,
                              const uint8_t* mask, void* stream);
int    sir_stream_input_push(sir_handle* h, void* state, size_t state_bytes, const sir_stream_input_config* cfg,
                             const void* in, int64_t in_stride, int in_width, const int32_t* in_lengths, const uint8_t* close,
                             float* out, int64_t out_stride, int32_t* out_lengths, void* stream);

/* The GRU recurrence kernels (forward and backward) exchange hidden-state slices between the workgroups of a
 * cluster through tagged granules in global memory and rely on the cluster being co-resident.  A workgroup that
 * spins past its limit (a partitioned / oversubscribed GPU, a stalled peer) sets a device status word owned by the
 * handle and carries on with invalid values.  sir_check_status waits for `stream`, returns SIR_ETIMEOUT if any
 * recurrence launched on this handle since the last check timed out (and clears the word), SIR_OK otherwise.
 * Call it wherever the host synchronises anyway -- once per batch of predictions (scripts/evaluate.py:85-86's
 * .cpu()) or per epoch (scripts/train.py:116's loss.item()); sir_profile_collect performs the same check.
 * The same word carries sir_ce_loss's / sir_ce_loss_soft's "label outside [0, num_classes)" flag (nn.CrossEntropyLoss raises on such a
 * target, train.py:242/:105; the kernel makes that step's loss NaN): reported here as SIR_EINVAL.  sir_eval_accumulate and
 * sir_temperature_fit raise it (bit 512) for such a label too.
 * The model's operand-range reports (see sir_model_infer) share the word, all SIR_EINVAL: bit 3 (value 8) a transformed conv2 / conv3
 * weight with |U| >= 32 or not finite; bit 11 (2048) a GRU weight matrix element beyond +-65504 or not finite; bit 12 (4096) a
 * training forward whose conv2 / conv3 block output reached 256 / 512 (the weight gradients of that workspace are invalid); bit 13
 * (8192) a conv1 weight or a BatchNorm weight / bias / running statistic that is not finite.  sir_decode_slots raises bit 14
 * (16384) for a tuple table with a label outside its slot (SIR_EINVAL). */
int sir_check_status(sir_handle* h, void* stream);

/* ---- cross-batch pipelining (owned by the library) ------------------------------------------------
 * One batch's kernels run back to back on one stream, and some of them cannot fill the chip on their own: the GRU
 * recurrence is a chain of S dependent steps that occupies half of the CUs at a fraction of their matrix throughput
 * (all utterances of the batch already advance in parallel inside it, so splitting a batch does not shorten the chain --
 * DESIGN.md section 4).  What hides it is the NEXT batch's convolutions.  A sir_pipeline owns n_slots HIP streams and the
 * events that order them against the caller's stream, so that a caller living on ONE stream gets the overlap:
 *     sir_pipeline_begin(p, caller_stream, &slot, &slot_stream)   -- slot = submission count mod n_slots; its stream now
 *                                                                    waits for everything queued on caller_stream
 *     sir_features_fwd(..., slot_stream); sir_model_infer(..., slot_stream);   (buffers / workspace of THAT slot)
 *     sir_pipeline_end(p, slot)                                   -- marks the slot's work complete-able
 *     ... more batches ...
 *     sir_pipeline_join(p, caller_stream)                         -- caller_stream waits for every slot (no host sync)
 * A slot's buffers are reused n_slots submissions later (same stream: ordered); the caller reads results on
 * caller_stream after the join.  n_slots = 1 degenerates to the caller's own stream.  Results are bit-identical to the
 * single-stream order.  Replaces nothing in the reference (its evaluate loop is serial, scripts/evaluate.py:79-86). */
typedef struct sir_pipeline sir_pipeline;
int sir_pipeline_create(sir_handle* h, int n_slots, sir_pipeline** out);     /* 1 <= n_slots <= 4 */
int sir_pipeline_destroy(sir_pipeline* p);
int sir_pipeline_begin(sir_pipeline* p, void* caller_stream, int* slot, void** slot_stream);
int sir_pipeline_end(sir_pipeline* p, int slot);
int sir_pipeline_join(sir_pipeline* p, void* caller_stream);

/* ---- training step ----------------------------------------------------------------------------
 * Replaces the body of train_epoch (scripts/train.py:90-107): model(mel) in train() mode,
 * criterion(output, label), loss.backward(), optimizer.step().
 * Gradients are written (not accumulated) to the device pointers of sir_model_grads, which mirror
 * the parameter pointers of sir_model_weights (the BN running statistics have no gradient). */
typedef struct sir_model_grads {
    float* conv_w[3];
    float* bn_w[3];
    float* bn_b[3];
    float* gru_w_ih[4];
    float* gru_w_hh[4];
    float* gru_b_ih[4];
    float* gru_b_hh[4];
    float* attn_w;
    float* attn_b;
    float* fc_w;
    float* fc_b;
} sir_model_grads;

/* Training-mode forward (models/models.py:41-68 under model.train()): BatchNorm uses batch
 * statistics and updates bn_running_mean/var IN PLACE (momentum, unbiased variance); the inter-layer
 * GRU dropout (models.py:32) uses a counter-based mask keyed by dropout_seed (dropout_p = 0 turns it
 * off); activations needed by the backward pass stay in `workspace`
 * (sir_model_workspace_bytes(h, batch, t_frames, 1) bytes), which must be handed unchanged to
 * sir_model_train_bwd.
 * Operand limits, non-finite features and weights: the paragraph at sir_model_infer (status bits 3, 11, 12, 13).
 * Batch regimes as at sir_model_infer (half chip at 256, full chip at 512, oversubscribed beyond); the step is tested against the float64
 * oracle at batches 257, 512, 528 and 1041 of 24 frames, and from 1 token (batch 1 of 8 frames; token count = batch * (t_frames / 8)) to
 * 10240 tokens (batch 405 of 200 frames, batch 40 of 2048: tests/test_token_range_gpu.py).  Batch 2048 of 256 frames runs with a clean
 * status word, finite results and conv2's weight gradient (there on the nine-tap fallback) checked on its own
 * (tests/test_conv_fallback_gpu.py).  Untested against the oracle of the whole step: token counts above 10240, and batches above 1100.
 * The backward's one shape limit inside the accepted range -- the conv2 / conv3 weight gradient of a long sequence in a very large
 * batch -- is stated at "Sequence regimes" (sir_model_infer). */
int sir_model_train_fwd(sir_handle* h, const sir_model_weights* w, float* const bn_running_mean[3],
                        float* const bn_running_var[3], const float* feats, int batch, int t_frames,
                        float bn_momentum, float dropout_p, uint64_t dropout_seed, float* logits,
                        void* workspace, size_t workspace_bytes, void* stream);

/* nn.CrossEntropyLoss() (mean) of train.py:242/105: loss[0] = -mean log softmax(logits)[label];
 * dlogits (optional) = d loss / d logits * grad_scale.  As torch's default ignore_index, a label of -100 takes its row out of
 * the loss, the gradient and the mean's divisor; any other label outside [0, num_classes) -- torch raises on it -- makes the
 * loss NaN and is reported by sir_check_status (SIR_EINVAL). */
int sir_ce_loss(sir_handle* h, const float* logits, const int64_t* labels, int batch, int num_classes,
                float* loss, float* dlogits, float grad_scale, void* stream);

/* sir_ce_loss with a soft target q_b = (1 - eps) * (lam_b * e[ya_b] + (1 - lam_b) * e[yb_b]) + eps / C:
 *   loss = mean over non-ignored rows of -sum_c q_b[c] * log softmax(logits_b)[c]
 *   dlogits_b = (softmax(logits_b) - q_b) * grad_scale / n_valid
 * i.e. what torch computes for lam * F.cross_entropy(l, ya, label_smoothing=eps) + (1 - lam) * F.cross_entropy(l, yb,
 * label_smoothing=eps) with a per-row lam (mixup's loss, and nn.CrossEntropyLoss(label_smoothing=eps) without labels_b).
 *   labels_b        : device int64[batch], NULL = no second label
 *   lam             : device f32[batch], NULL = all 1; read only when labels_b is given
 *   label_smoothing : host float in [0, 1) (else SIR_EINVAL)
 * A row is ignored iff labels_a[b] == -100 (labels_b of such a row is not read); any other label of either array outside
 * [0, num_classes) makes the loss NaN and is reported by sir_check_status (SIR_EINVAL), as for sir_ce_loss.  With
 * labels_b == NULL and label_smoothing == 0 the results are bit-identical to sir_ce_loss (the same kernel is launched). */
int sir_ce_loss_soft(sir_handle* h, const float* logits, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                     float label_smoothing, int batch, int num_classes, float* loss, float* dlogits, float grad_scale,
                     void* stream);

/* loss.backward() (train.py:106): all 29 parameter gradients from dlogits and the saved workspace.  dlogits may have any finite
 * magnitude (the internal loss scale follows max |dlogits|: slot 39 below, and the paragraph at sir_model_infer).
 * SIR_EUNSUPPORTED, before anything is launched or written, when a wanted conv2 / conv3 weight gradient falls into the one corner of
 * batch * t_frames the kernels do not cover ("Sequence regimes" at sir_model_infer); this holds for every form of the backward below. */
int sir_model_train_bwd(sir_handle* h, const sir_model_weights* w, const float* feats, const float* dlogits,
                        int batch, int t_frames, float dropout_p, uint64_t dropout_seed,
                        const sir_model_grads* grads, void* workspace, size_t workspace_bytes, void* stream);
/* The same backward in two halves, for data-parallel training that starts the gradient exchange early (SURVEY.md
 * section 8(e)): SIR_BWD_HEAD_GRU writes the fc / attention / GRU gradients (96 % of the bytes; they are final after this
 * call) and leaves d(loss)/d(GRU input) in the workspace; SIR_BWD_CNN, called next on the same workspace, writes the
 * conv / BatchNorm gradients.  SIR_BWD_ALL = sir_model_train_bwd. */
#define SIR_BWD_ALL 0
#define SIR_BWD_HEAD_GRU 1
#define SIR_BWD_CNN 2
int sir_model_train_bwd_part(sir_handle* h, const sir_model_weights* w, const float* feats, const float* dlogits,
                             int batch, int t_frames, float dropout_p, uint64_t dropout_seed,
                             const sir_model_grads* grads, void* workspace, size_t workspace_bytes, int part,
                             void* stream);
/* Byte offsets of the training workspace's slots for one shape (debugging and tests: the library's own calls need none of
 * this).  Writes min(n, slot count) offsets and returns the slot count; touches no device (`h` may be NULL).  Every slot is
 * 256-byte aligned; fp32 unless noted; B = batch, S = t_frames / 8 GRU steps, wp1 = t_frames / 2, wp2 = t_frames / 4.
 * Indices are stable: slots are appended, never renumbered.
 *    0  a1     conv1 block output (pooled)         [B][32][wp1][32]
 *    1  z2     conv2 raw output                    [B][32][wp1][64]
 *    2  a2     conv2 block output                  [B][16][wp2][64]
 *    3  z3     conv3 raw output                    [B][16][wp2][128]
 *    4  x0     conv3 block output = GRU layer 0 input   [B][S][1024]
 *    5  gi     input projection of the running layer    [B][S][1536]
 *    6  g0     saved gates of GRU layer 0          [B][S][2][4][256]
 *    7  g1     saved gates of GRU layer 1
 *    8  y0     GRU layer 0 output                  [B][S][512]
 *    9  y0d    layer 0 output behind the dropout   [B][S][512]
 *   10  y1     GRU layer 1 output                  [B][S][512]
 *   11  ctx    attention-pooled context            [B][512]
 *   12  bn     BatchNorm scale, shift, mean, invstd     [4][224] (bn1 | bn2 | bn3 at channels 0, 32, 96)
 *   13  bnb    backward: mean dy, mean dy * xhat   [2][224]
 *   14  stats  partial sums of the BatchNorm reductions (float2)
 *   15, 16     reserved
 *   17  wht    W_hh as the forward recurrence's resident fragments
 *   18  wr4    W_hh as the backward recurrence's resident fragments
 *   19, 20     reserved
 *   21  dy1    gradient of y1                      [B][S][512]
 *   22  dy0    gradient of y0                      [B][S][512]
 *   23  dgi    gate gradients of layer 0, input side    [B][S][1536]
 *   24  dgh    gate gradients of layer 0, hidden side   [B][S][1536]
 *   25  dx0    gradient of x0                      [B][S][1024]
 *   26  dz3    gradient of z3
 *   27  da2    gradient of a2
 *   28  dz2    gradient of z2
 *   29  da1    gradient of a1
 *   30  small  attention-gradient and conv1-backward partials
 *   31  slab   split-K / weight-gradient slabs
 *   32  xs     16-bit planes of the input-projection GEMM's A operand
 *   33  ws     16-bit planes of W_ih (both layers, both directions)
 *   34  wcb    16-bit planes of the conv2 / conv3 weights (forward and data-gradient forms)
 *   35  c1m    conv1 input moments (54 doubles)
 *   36  dgi1   gate gradients of layer 1, input side
 *   37  dgh1   gate gradients of layer 1, hidden side
 *   38  slab2  GRU weight-gradient slabs of the side stream
 *   39  bsc    the backward's loss scale as pairs {scale, 1 / scale} of powers of two, [1 + B][2]: pair 0 is the call's (from the
 *              maximum of |dlogits|; the static 2^8 x batch, rounded up to a power of two, while that maximum times the static
 *              scale lies in [2^5, 2^10), else the power of two that puts it into [2^7, 2^8)); pair 1 + b is utterance b's own,
 *              written and used only by a sir_model_train_bwd_x call with all three bn_frozen set and no parameter gradient wanted
 *              (rows are then independent, and each is scaled by its own row of dlogits).  Slots 21..29 carry the scale.
 *              With a gradient at the embedding (sir_model_train_bwd_emb, demb != NULL) the maximum is max(|dlogits|, |demb| * 2^5),
 *              over the call or over row b of both: the head adds demb to dctx = dlogits fc_w, and at the reference head's
 *              initialisation (fc_w uniform within +-512^-1/2 = 2^-4.5) max |dctx| is about max |dlogits| * 2^-4.5, so a demb of
 *              magnitude m loads the fp16 contractions behind the head like a dlogits of m * 2^4.5 -- rounded up to 2^5, the
 *              side that scales down.  With dlogits all zero the scale follows demb alone.  demb == NULL: the pairs of before.
 *   40  rag    the ragged step (sir_model_train_fwd_ragged): int32 [4][B] -- the validated frames (0 for a length outside [8, T]),
 *              W1, W2 and S_b of every clip; written by that call and rewritten by sir_model_train_bwd_ragged, untouched otherwise */
int sir_model_train_workspace_offsets(const sir_handle* h, int batch, int t_frames, size_t* offsets, int n);

/* ---- fine-tuning step -------------------------------------------------------------------------
 * The torch recipe for adapting a checkpoint: model.train(), then bnK.eval() for the blocks whose pretrained statistics
 * are kept and p.requires_grad_(False) for the layers that stay fixed.
 *   bn_frozen[k] != 0 : BatchNorm k+1 normalises with bn_running_mean / bn_running_var (and eps) and does not touch them;
 *                       its backward is the affine form dz = dy * gamma * invstd_running (no mean terms),
 *                       dgamma = sum dy * xhat (xhat from the running statistics), dbeta = sum dy.
 * The three flags are independent.  cfg == NULL means {0, 0, 0}: exactly sir_model_train_fwd / _bwd_part. */
typedef struct sir_train_config {
    int bn_frozen[3];
} sir_train_config;

/* sir_model_train_fwd with per-block frozen statistics.  For a frozen block the statistics work is not launched
 * (conv1: the input-moment kernels; conv2 / conv3: the finalise pass); one small kernel folds the running statistics
 * into the per-channel scale / shift / mean / invstd arrays the apply kernels and the backward read. */
int sir_model_train_fwd_cfg(sir_handle* h, const sir_model_weights* w, float* const bn_running_mean[3],
                            float* const bn_running_var[3], const float* feats, int batch, int t_frames,
                            float bn_momentum, float dropout_p, uint64_t dropout_seed, const sir_train_config* cfg,
                            float* logits, void* workspace, size_t workspace_bytes, void* stream);
/* sir_model_train_bwd_part for the workspace a sir_model_train_fwd_cfg call with the SAME cfg left behind.  A NULL pointer
 * in `grads` means "not wanted": the chain head -> GRU layer 1 -> GRU layer 0 -> conv3 -> conv2 -> conv1 stops below the
 * lowest block that still has a wanted gradient, and a launch that only feeds unwanted gradients is not issued (the four
 * weight-gradient GEMMs of a GRU layer, its bias sums, a convolution's weight gradient, a frozen BatchNorm's reduce, the
 * layer-0 input gradient and everything under it when no conv / bn gradient is wanted).  Where one launch writes wanted
 * and unwanted gradients the unwanted stores are left out.  Every wanted gradient is bit-identical to
 * what the call writes for it with no NULL pointer and the same cfg.  `part` as for sir_model_train_bwd_part. */
int sir_model_train_bwd_cfg(sir_handle* h, const sir_model_weights* w, const float* feats, const float* dlogits,
                            int batch, int t_frames, float dropout_p, uint64_t dropout_seed,
                            const sir_train_config* cfg, const sir_model_grads* grads, void* workspace,
                            size_t workspace_bytes, int part, void* stream);

/* ---- gradient with respect to the input features ------------------------------------------------
 * sir_model_train_bwd_cfg that also returns d(loss)/d(feats): what torch leaves in x.grad after
 *     x.requires_grad_(True); loss = criterion(model(x), label); loss.backward()
 * (saliency maps, FGSM-style robustness checks, a differentiable stage in front of the model).
 *   dfeats : device f32 [batch][64][t_frames], the layout of feats; written (not accumulated), without the backward's
 *            internal loss scale; a buffer of its own.  NULL: the call IS sir_model_train_bwd_cfg -- same launches, same bits.
 * With dfeats the data chain head -> GRU 1 -> GRU 0 -> conv3 -> conv2 -> conv1 runs to the bottom whatever `grads` holds:
 * all 29 pointers NULL is legal and launches no weight-gradient GEMM, no bias sum and no convolution weight gradient.  Every
 * wanted parameter gradient is bit-identical to what the call writes for it with dfeats == NULL.  The last link is one
 * kernel: dz1 = d(loss)/d(conv1 output) is recomputed per tile from feats and da1 (slot 29) -- conv1's nine-fma chain, the
 * BatchNorm fold of slot 12, the forward's ReLU / max-pool routing -- and convolved with the transposed taps; it is never
 * stored.  With live bn1 statistics conv1's reduce pass runs even when no conv1 / bn1 gradient is wanted (its parameter
 * stores are then left out) and leaves mean dy, mean dy * xhat of bn1 in channels 0..31 of slot 13; with bn_frozen[0] and
 * no conv1 / bn1 gradient wanted it is not launched.
 *   part : SIR_BWD_ALL and SIR_BWD_CNN write dfeats; SIR_BWD_HEAD_GRU ignores it (but runs the chain down to dx0, slot 25,
 *          which the SIR_BWD_CNN call that follows reads).  Both halves of a split call must get the same dfeats-or-NULL.
 * Every argument is validated before anything is launched. */
int sir_model_train_bwd_x(sir_handle* h, const sir_model_weights* w, const float* feats, const float* dlogits,
                          int batch, int t_frames, float dropout_p, uint64_t dropout_seed,
                          const sir_train_config* cfg, const sir_model_grads* grads, float* dfeats,
                          void* workspace, size_t workspace_bytes, int part, void* stream);

/* ---- the ragged (un-padded) differentiable step --------------------------------------------------
 * sir_model_infer_ragged's function, differentiable: row b of the logits is what the model gives feats[b][:, :frames[b]] on its
 * own -- every BatchNorm on its running statistics, the GRU in training mode (the inter-layer dropout mask of the padded step: same
 * hash, same element index (b * S + t) * 512 + u, applied for t < S_b), the attention softmax over t < S_b -- and the backward is
 * the gradient of that function.  Widths as for sir_model_infer_ragged: W1 = frames / 2, W2 = W1 / 2, S_b = W2 / 2.
 *   frames : device int32 [batch], each in [8, t_frames].  A value outside it behaves as in inference: the clip's width counts as 0,
 *            row b of the logits is NaN and status bit 6 is raised (SIR_EINVAL at the next sir_check_status); the backward treats
 *            that row's dlogits as zero and writes a zero dfeats row.  Whatever frames holds, nothing is read or written out of
 *            bounds.  Feature columns >= frames[b] are never read as data.
 *   cfg    : must set all three bn_frozen.  Anything else, NULL included, is SIR_EUNSUPPORTED before any launch: with batch
 *            statistics a clip has no result of its own.  The running statistics are read, never written.
 *   workspace : the one sir_model_workspace_bytes(h, batch, t_frames, 1) sizes; slot 40 (appended) holds the validated frames and
 *            the three widths of every clip as int32 [4][batch].  Behind a clip's widths a1, a2, x0 (slots 0, 2, 4), y0, y0d, y1
 *            (8, 9, 10) and every gradient slot are zeros; the saved gates (6, 7) and z2 / z3 (1, 3) are unspecified there.
 * The chain: the ragged conv1 kernel of inference (+ zeros behind W1), conv2 / conv3 and both input projections at full width on
 * maps that are zero behind the clip (their kernels, the conv fallback route included, are the padded step's), the BN + ReLU + pool
 * kernels writing zeros behind W2 / S_b, the ragged form of the recurrence that saves its gates, the ragged attention kernel.
 * Backward: a length-aware head, the BPTT kernel's ragged form (all S steps under a predicate: zero gate gradients and a held /
 * dropped carry for t >= S_b, no saved row of such a step used as data), width masks on the pooled gradients (the transposed
 * convolutions spill one column past a clip's width) in the BatchNorm backward, its frozen dgamma / dbeta sums and conv1's two
 * kernels, which also write dfeats as zero at columns >= frames[b].  No atomics, fixed summation order: bit-reproducible, and the
 * one- and two-stream forms agree.
 * sir_model_train_bwd_ragged: `grads` with the pruning rules of sir_model_train_bwd_cfg, `dfeats` as for sir_model_train_bwd_x,
 * `part` as for sir_model_train_bwd_part; frames, cfg, dropout_p and dropout_seed those of the forward call.
 * Every argument is validated before anything is launched or written. */
int sir_model_train_fwd_ragged(sir_handle* h, const sir_model_weights* w, const float* const bn_running_mean[3],
                               const float* const bn_running_var[3], const float* feats, const int32_t* frames, int batch,
                               int t_frames, float dropout_p, uint64_t dropout_seed, const sir_train_config* cfg,
                               float* logits, void* workspace, size_t workspace_bytes, void* stream);
int sir_model_train_bwd_ragged(sir_handle* h, const sir_model_weights* w, const float* feats, const int32_t* frames,
                               const float* dlogits, int batch, int t_frames, float dropout_p, uint64_t dropout_seed,
                               const sir_train_config* cfg, const sir_model_grads* grads, float* dfeats, void* workspace,
                               size_t workspace_bytes, int part, void* stream);

/* ---- a second gradient entrance, at the embedding ------------------------------------------------
 * The superset of the backward forms above, for a loss that is put on the 512-float attention-pooled context itself
 * (sir_proxy_loss) alone or beside the classifier's: frames == NULL is sir_model_train_bwd_x (cfg == NULL: every BatchNorm live),
 * frames != NULL is sir_model_train_bwd_ragged with its rules for cfg.
 *   demb    : device f32 [batch][512] = d(loss)/d(ctx), unscaled like dlogits, 16-byte aligned.  The head adds row b of it to the
 *             dctx it forms from dlogits (dctx = dlogits fc_w + demb); dy1, the attention gradients, the GRU, the CNN and dfeats
 *             follow unchanged.  It does not enter the fc weight / bias gradient.  NULL: the call IS the form above for that
 *             combination -- same launches, same bits, slot 39 included.
 *   dlogits : required as before; a caller without a classifier loss passes zeros.
 * Ragged: a clip with S_b < 1 ignores its demb row as it ignores its dlogits row (a NaN there does not travel).
 * The call's loss scale (slot 39) takes max(|dlogits|, |demb| * 2^5) where it took max |dlogits| -- over the call, or in the
 * per-row mode over row b of both -- so a demb of any finite magnitude, with dlogits zero or not, is as accurate as a dlogits
 * of the usual one.  Every argument is validated before anything is launched or written. */
int sir_model_train_bwd_emb(sir_handle* h, const sir_model_weights* w, const float* feats, const int32_t* frames /* NULL: padded */,
                            const float* dlogits, const float* demb /* or NULL */, int batch, int t_frames, float dropout_p,
                            uint64_t dropout_seed, const sir_train_config* cfg, const sir_model_grads* grads,
                            float* dfeats /* or NULL */, void* workspace, size_t workspace_bytes, int part, void* stream);

/* optimizer.step() for torch.optim.Adam(lr, betas, eps, weight_decay) with coupled L2
 * (train.py:246-250, :107): one multi-tensor launch.  The pointer arrays are HOST arrays of device
 * pointers (n_tensors <= 32); `step` is the 1-based step count used for bias correction. */
int sir_adam_step(sir_handle* h, int n_tensors, float* const* params, const float* const* grads,
                  float* const* exp_avg, float* const* exp_avg_sq, const int64_t* sizes, int step,
                  float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* ---- gradient norm and clipping ----------------------------------------------------------------
 * torch.nn.utils.clip_grad_norm_(parameters, max_norm) (norm_type 2, error_if_nonfinite=False) between loss.backward() and
 * optimizer.step(); the reference's configs/config.yaml carries an unread `grad_clip`.  The gradient tensors are described
 * as for sir_adam_step (HOST arrays of device pointers and element counts, n_tensors <= 32).
 * sir_grad_norm_partials: host helper, the number of floats `partials` must hold (one per 4096-element chunk of every
 *   tensor); -1 on bad input.  The library allocates nothing.
 * sir_grad_norm: launch 1 writes one fp32 sum of squares per chunk into `partials` (ordered in-block reduction).  Launch 2
 *   sums the partials in index order in double and writes out2 = {total_norm, coef} (device f32[2]),
 *   coef = min(1, max_norm / (total_norm + 1e-6)); with scale_in_place != 0 it runs over the gradients' grid, every
 *   workgroup forms the same sum itself and multiplies its chunk by coef (torch's in-place semantics: a non-finite norm
 *   leaves non-finite gradients; nothing is skipped).  No atomics: the norm is bit-reproducible run to run.
 *   out2 == NULL (scale_in_place must be 0): launch 1 only -- the partials are then consumed by sir_adam_step_clipped.
 *   max_norm <= 0 or NaN: SIR_EINVAL (not looked at when out2 == NULL); partials_floats too small: SIR_ENOMEM.
 * sir_adam_step_clipped: sir_adam_step on g * coef (rounded to fp32, taken before the weight-decay term -- the order of
 *   clip_grad_norm_ followed by optimizer.step()), coef formed from `partials` (n_partials floats, as sir_grad_norm left
 *   them for the SAME tensors) exactly as sir_grad_norm forms it.  The gradient buffers are left unscaled; workgroup 0
 *   writes out2 = {total_norm, coef}.  Nothing synchronises with the host: coef never leaves the device. */
int sir_grad_norm_partials(int n_tensors, const int64_t* sizes);
int sir_grad_norm(sir_handle* h, int n_tensors, float* const* grads, const int64_t* sizes, float max_norm, float* partials,
                  int partials_floats, float* out2, int scale_in_place, void* stream);
int sir_adam_step_clipped(sir_handle* h, int n_tensors, float* const* params, const float* const* grads,
                          float* const* exp_avg, float* const* exp_avg_sq, const int64_t* sizes, int step, float lr,
                          float beta1, float beta2, float eps, float weight_decay, const float* partials, int n_partials,
                          float max_norm, float* out2, void* stream);

/* ---- every variant of the optimizer step --------------------------------------------------------
 * sir_adam_step_ex: one multi-tensor launch for torch.optim.Adam / torch.optim.AdamW, with or without the clip coefficient of
 * sir_adam_step_clipped, with or without an exponential moving average ("shadow") of the parameters updated in the same
 * pass.  Tensors as for sir_adam_step (HOST arrays of device pointers and element counts, n_tensors <= 32).
 *   decoupled == 0, ema_decay == 0: the call IS sir_adam_step (max_norm == 0) or sir_adam_step_clipped (max_norm > 0): the same
 *     kernel, the same bits.
 *   decoupled != 0: p is first multiplied by (float)(1.0 - (double)lr * (double)weight_decay), formed on the host; the Adam
 *     update then runs on the gradient alone (clipped if asked for), no weight_decay * p term: torch.optim.AdamW's order.
 *   ema_decay = d in (0, 1): ema[i] = fmaf(d, ema[i], (1.0f - d) * p_new) with the parameter value the step has just formed.
 *     d is read per call (the host may warm it up).  `ema` holds n_tensors device pointers, none NULL, none aliasing its
 *     parameter; ema must be NULL when ema_decay == 0.  The caller initialises the shadow (a copy of the parameters).
 *   max_norm > 0: `partials` / `n_partials` / `out2` as for sir_adam_step_clipped; max_norm == 0: they are not read.
 * SIR_EINVAL: NaN in any float of cfg, ema_decay outside [0, 1), ema == NULL with ema_decay > 0 (or the reverse),
 * max_norm < 0, max_norm > 0 without partials / out2.  The library allocates nothing. */
typedef struct sir_adam_config {
    float lr, beta1, beta2, eps, weight_decay;
    int   decoupled;      /* 0: coupled L2 (torch.optim.Adam); 1: torch.optim.AdamW */
    float max_norm;       /* 0 = no clipping; > 0: as sir_adam_step_clipped (partials / n_partials / out2 required) */
    float ema_decay;      /* 0 = no shadow; in (0, 1): shadow update with THIS step's decay */
} sir_adam_config;
int sir_adam_step_ex(sir_handle* h, int n_tensors, float* const* params, const float* const* grads,
                     float* const* exp_avg, float* const* exp_avg_sq, float* const* ema /* NULL iff ema_decay == 0 */,
                     const int64_t* sizes, int step, const sir_adam_config* cfg,
                     const float* partials, int n_partials, float* out2, void* stream);

/* ---- classification and evaluation of logits (csrc/evaluate.hip) ----------------------------------
 * What follows the forward pass, for a whole batch on the device: softmax + top-k (sir_classify), the counts and sums an
 * evaluation report is made of (sir_eval_accumulate) and temperature scaling (sir_temperature_fit; Guo et al. 2017).
 * Common to the calls: logits [rows][num_classes] f32, 4-byte aligned, 1 <= num_classes <= 64 (as sir_model_weights),
 * 1 <= rows <= 2^30 (sir_temperature_fit: 2^22), anything else SIR_EINVAL;
 * one wavefront per row, one lane per class.  Nothing allocates, nothing synchronises with the host, only kernels are
 * launched (legal under stream capture), and every argument is checked before the first launch: a refused call writes nothing.
 *   inv_temperature : DEVICE f32[1], beta = 1 / T, > 0; NULL = 1.
 *   order           : classes rank by descending logit, equal logits by ascending class index.  Rank 0 is therefore the
 *                     "first maximum" sir_model_infer's argmax returns, on every finite row, whatever beta > 0 is.
 *   softmax         : p = softmax(l * beta) as p = exp(d) / den with d = (l - max l) * beta -- the row maximum is subtracted first,
 *                     then one product -- den = 1 + rest, rest = the sum of exp(d) over every class but the first maximum
 *                     (whose term is exactly 1), all in fp32; log den is taken as log1pf(rest).
 *   non-finite row  : a row that holds a NaN or an infinity (tested on the logits themselves, not on l * beta).
 *
 * sir_classify: probs (optional, [batch][num_classes]) = p; topk_idx int32 [batch][k] / topk_prob f32 [batch][k] = the classes
 *   of rank 0 .. k - 1 and their p.  1 <= k <= min(8, num_classes), else SIR_EINVAL.  A non-finite row yields NaN in probs and
 *   topk_prob and -1 in topk_idx; the other rows are unaffected.
 *
 * sir_eval_accumulate adds one batch into `state`, a caller-owned device buffer of sir_eval_state_bytes(num_classes, n_bins)
 *   bytes (0 for arguments out of range), 8-byte aligned, zeroed by the caller before the first batch.  1 <= n_bins <= 64.
 *   A smaller state_bytes is SIR_ENOMEM.  Layout, every field 8 bytes wide, in this order (C = num_classes, M = n_bins):
 *     int64  confusion[C][C]   row = true label, column = predicted class (rank 0)
 *     int64  n                 rows counted
 *     int64  topk_correct[8]   entry j: rows whose label has rank < min(j + 1, C)
 *     double nll_sum           sum of -log p[label], per row log1pf(rest) - d[label] in fp32
 *     int64  bin_count[M]      rows by confidence bin: min(M - 1, (int)floorf(p_max * M)), p_max = p of rank 0, fp32
 *     int64  bin_correct[M]    of those, the rows whose prediction is the label
 *     double bin_conf_sum[M]   sum of p_max over the bin's rows
 *     int64  n_ignored         rows whose label is -100 (nn.CrossEntropyLoss's ignore_index, as sir_ce_loss)
 *     int64  n_nonfinite       rows with a valid label and a non-finite logit row
 *     double scratch[64][M+1]  the call's own workspace (per workgroup {NLL partial, bin_conf_sum partials}); need not be zero,
 *                              holds nothing a caller reads
 *   A row is looked at in this order: label -100 -> n_ignored and nothing else; any other label outside [0, C) -> no field
 *   moves and the handle's status word is raised (SIR_EINVAL at the next sir_check_status, as sir_ce_loss); a non-finite row ->
 *   n_nonfinite and nothing else; every other row counts in all remaining fields.
 *   The integer fields are added with integer atomics (exact, order-independent).  The doubles are summed in a fixed order -- G =
 *   min(64, ceil(batch / 16)) workgroups of 16 waves, wave g of the 16 G takes rows g, g + 16 G, ...; a workgroup's 16 wave sums
 *   are added in wave order into its partial (scratch), and a second single-workgroup launch adds the G partials in order to
 *   the state -- with no floating-point atomic: bit-reproducible run to run.  Calls into one state add up; they must be
 *   ordered (one stream, or events).
 *
 * sir_temperature_fit minimises f(beta) = mean_i [logsumexp(beta l_i) - beta l_{i, y_i}] over beta = 1 / T (convex:
 *   f' = mean(E_p[l] - l_y), f'' = mean(Var_p(l)), p = softmax(beta l)).  From beta = 1 it runs `iters` (0 .. 1000; 20 is plenty)
 *   safeguarded Newton steps  b = clamp(beta - f' / max(f'', 1e-12), beta / 2, 2 beta), beta = (float)clamp(b, 1/64, 64), the
 *   step evaluated in double; a NaN step keeps beta.  Each step is one reduction launch (per-row terms in fp32 on the centred
 *   logits c = l - max l: log1pf(rest) - beta c_y, E_p[c] - c_y, E_p[(c - E_p[c])^2]; sums over rows in double in a fixed
 *   order: run-to-run reproducible) and one single-thread update launch; beta
 *   never leaves the device.  Rows are left out (label -100, non-finite row) or flagged (other label outside [0, C)) as by
 *   sir_eval_accumulate; the means run over the remaining rows (none left: beta stays 1, the two nll are NaN).
 *   out       : device f32[3] = {beta, f(1), f(beta)}; out (also out + 0 alone) may be passed on as inv_temperature
 *   n_rows    : 1 .. 2^22
 *   workspace : sir_temperature_fit_workspace_bytes(n_rows) bytes, 8-byte aligned (too small: SIR_ENOMEM); contents need not
 *               be initialised */
int sir_classify(sir_handle* h, const float* logits, int batch, int num_classes, const float* inv_temperature, int k,
                 float* probs, int32_t* topk_idx, float* topk_prob, void* stream);
size_t sir_eval_state_bytes(int num_classes, int n_bins);
int sir_eval_accumulate(sir_handle* h, const float* logits, const int64_t* labels, int batch, int num_classes,
                        const float* inv_temperature, int n_bins, void* state, size_t state_bytes, void* stream);
size_t sir_temperature_fit_workspace_bytes(int n_rows);
int sir_temperature_fit(sir_handle* h, const float* logits, const int64_t* labels, int n_rows, int num_classes, int iters,
                        float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- slot heads: one logit row as several independent softmax segments (DESIGN.md section 4 "Slot heads") --------------
 * A slot layout is n_slots (1 .. 8) segment widths C_0 .. C_{G-1}, each >= 1, with sum C_g == num_classes <= 64.  Slot g owns
 * the logit columns [start_g, start_g + C_g), start_g = the sum of the widths before it.  Labels are int64 [batch][n_slots],
 * row-major; entry g lies in [0, C_g), local to the slot, or is -100.  The model is unchanged (fc writes the num_classes logits);
 * sir_model_infer's argmax stays the argmax over the WHOLE row, which means nothing under a slot layout.
 * Common to the calls below, as to their single-head relatives:
 *   slot_sizes : HOST int32[n_slots].
 *   Every argument is checked before the first launch -- the layout rules above, the sum against num_classes, NULLs, alignment
 *   (f32 / int32 pointers 4 bytes, int64 labels and the state 8 bytes), k -- and a refused call (SIR_EINVAL; a too small state
 *   SIR_ENOMEM) writes nothing.  Only kernels are launched (legal under stream capture), nothing allocates, nothing
 *   synchronises with the host.  No floating-point atomics: results are bit-reproducible run to run.
 *   Per slot the arithmetic is the single-head call's arithmetic on the segment; what is promised below as "bit-identical to
 *   X on a contiguous copy of the segment" means X called with logits = the [batch][C_g] copy of the segment's columns, labels =
 *   column g of the labels, num_classes = C_g.
 *
 * sir_ce_loss_slots: sum over slots of weighted soft-target cross-entropies.
 *   labels_a, labels_b : device int64 [batch][n_slots]; labels_b NULL = no second label
 *   lam                : device f32[batch], NULL = all 1, read only when labels_b is given; one value per row for all its slots
 *   label_smoothing    : host float eps in [0, 1); slot g is smoothed with eps / C_g
 *   slot_weights       : HOST f32[n_slots], finite and >= 0 (else SIR_EINVAL); NULL = all 1
 *   slot_loss          : optional, device f32[n_slots]: entry g = the mean over the rows whose labels_a[b][g] != -100 of the
 *                        soft-target cross-entropy of segment g -- sir_ce_loss_soft's loss on that segment (no such row: NaN)
 *   loss               : device f32[1] = sum_g w_g * slot_loss[g]: fp32 products added in fp32 in slot order, starting from +0
 *   dlogits            : optional, [batch][num_classes]; segment g = what sir_ce_loss_soft writes for that segment with
 *                        grad_scale replaced by the fp32 product grad_scale * w_g (a zero weight: zeros on finite logits)
 *   A -100 in slot g takes the row out of slot g only: zeros in that segment of dlogits, not in that slot's divisor.  Any other
 *   label of either array outside [0, C_g) makes slot_loss[g] and loss NaN and is reported by sir_check_status (SIR_EINVAL),
 *   as for sir_ce_loss.  slot_loss[g] and segment g of dlogits are bit-identical to sir_ce_loss_soft on a contiguous copy of
 *   the segment (which, with labels_b == NULL and label_smoothing == 0, is sir_ce_loss); with n_slots == 1 and a NULL or unit
 *   weight so is loss.  One workgroup of 256 threads walks the slots in order, one thread per row as sir_ce_loss; widths <= 32
 *   and > 32 take the register-array lengths sir_ce_loss takes for them and may be mixed in one layout.
 *
 * sir_classify_slots: segment-wise softmax + top-k, one wavefront per row walking its slots.
 *   inv_temperature : DEVICE f32[n_slots], one beta per slot; NULL = all 1
 *   probs           : optional, [batch][num_classes] = the segment-wise softmax
 *   topk_idx        : int32 [batch][n_slots][k], topk_prob f32 [batch][n_slots][k], 1 <= k <= 8.  Indices are LOCAL to the slot;
 *                     ranks >= C_g hold -1 / 0.  Order and softmax are sir_classify's (descending logit, ties by ascending
 *                     index, den = 1 + rest).
 *   joint_prob      : optional, f32[batch] = the fp32 product, in slot order, of the slots' rank-0 probabilities
 *   A NaN or an infinity in segment g of a row makes that slot's outputs of the row NaN / -1 (all k ranks) and the row's
 *   joint_prob NaN; its other slots and all other rows are unaffected.  Per slot the outputs are bit-identical to sir_classify
 *   on a contiguous copy of the segment with that slot's beta.
 *
 * sir_eval_accumulate_slots adds one batch into `state`, a caller-owned, 8-byte aligned device buffer of
 *   sir_eval_slots_state_bytes(slot_sizes, n_slots, n_bins) bytes (0 for arguments out of range), zeroed by the caller before
 *   the first batch.  1 <= n_bins <= 64.  The state is n_slots single-head states back to back -- state g has exactly the
 *   layout of sir_eval_state_bytes(C_g, n_bins), scratch included -- followed by one joint block, every field 8 bytes wide
 *   (M = n_bins):
 *     int64  n                  rows counted jointly
 *     int64  exact_match        of those, the rows whose every slot's prediction (rank 0) is its label
 *     int64  slots_correct[9]   entry j: counted rows with exactly j slots right (entries above n_slots stay 0)
 *     double nll_sum            per counted row the double sum, in slot order, of the slots' fp32 terms log1pf(rest) - d[label]
 *     int64  bin_count[M]       counted rows by joint confidence: min(M - 1, (int)floorf(joint_prob * M)), joint_prob as
 *                               sir_classify_slots forms it
 *     int64  bin_correct[M]     of those, the exact matches
 *     double bin_conf_sum[M]    sum of joint_prob over the bin's rows
 *     int64  n_excluded         rows not counted jointly
 *     double scratch[64][M+1]   the call's own workspace, as in the single-head state
 *   Slot state g treats row b by labels[b][g] and segment g exactly as sir_eval_accumulate does (n_ignored, bad label -> status
 *   word, n_nonfinite, counted), with inv_temperature[g] (DEVICE f32[n_slots], NULL = all 1); after identical call sequences
 *   its integer fields and doubles are bit-identical to sir_eval_accumulate on contiguous copies.  A row counts in the joint
 *   block iff every slot has a label in [0, C_g) and a finite segment; every other row goes to n_excluded only.  Integer
 *   fields: integer atomics.  Doubles: the fixed-order scheme of sir_eval_accumulate (the same workgroup and wave map, per slot
 *   and for the joint block; a closing launch adds the workgroups' partials in order).  Calls into one state must be ordered. */
int sir_ce_loss_slots(sir_handle* h, const float* logits, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                      float label_smoothing, const int32_t* slot_sizes, const float* slot_weights, int n_slots, int batch,
                      int num_classes, float* loss, float* slot_loss, float* dlogits, float grad_scale, void* stream);
int sir_classify_slots(sir_handle* h, const float* logits, int batch, int num_classes, const int32_t* slot_sizes, int n_slots,
                       const float* inv_temperature, int k, float* probs, int32_t* topk_idx, float* topk_prob, float* joint_prob,
                       void* stream);
size_t sir_eval_slots_state_bytes(const int32_t* slot_sizes, int n_slots, int n_bins);
int sir_eval_accumulate_slots(sir_handle* h, const float* logits, const int64_t* labels, int batch, int num_classes,
                              const int32_t* slot_sizes, int n_slots, const float* inv_temperature, int n_bins, void* state,
                              size_t state_bytes, void* stream);

/* sir_decode_slots: the k best label TUPLES of every row (DESIGN.md section 4 "Joint decoding"), 1 <= k <= 8, in one launch; one
 * wavefront per row, nothing allocated, no floating-point atomics, results bit-reproducible.  slot_sizes (HOST) and
 * inv_temperature (DEVICE f32[n_slots] or NULL) as above.  Every argument is checked before the launch: a refused call
 * (SIR_EINVAL) writes nothing.
 *   Per row and slot lp_g[c] = d_c - log1pf(rest_g), d and rest as sir_classify_slots forms them: the fp32 terms of
 *   sir_eval_accumulate_slots' nll_sum, negated.  A tuple's score is s_t = lp_0[t_0] + lp_1[t_1] + ..., added in fp32 in slot
 *   order (no fma, no reassociation).
 *   Constrained (tuples != NULL, 1 <= n_tuples <= 4096): tuples is DEVICE uint8 [n_tuples][8], 8-byte aligned; byte g of a row
 *   is the slot-local label of slot g, bytes g >= n_slots are 0.  Ranking: descending s_t, equal bits by ascending table row.
 *     best_index  int32 [batch][k]           the table row
 *     best_labels int32 [batch][k][n_slots]  that tuple, unpacked
 *     best_logp   f32   [batch][k]           s_t
 *     best_prob   f32   [batch][k]           exp(s_t - L), L = logsumexp_t s_t over the table = max + log of a sum taken in a
 *                                            fixed lane (t = lane, lane + 64, ...) and butterfly order
 *     valid_mass  f32   [batch], optional    exp(L): the probability the independent heads put on tuples that exist
 *     tuple_logp  f32   [batch][n_tuples], optional   every s_t
 *   Ranks >= n_tuples hold -1 / -1 / -inf / 0.  A table byte >= C_g (g < n_slots) raises the status word (bit 14, 16384:
 *   SIR_EINVAL at the next sir_check_status); that tuple scores -inf, takes no part in L and is never chosen.
 *   Unconstrained (tuples == NULL, n_tuples == 0, tuple_logp == NULL): the k best tuples of the whole product space by staged
 *   merging (the k best partial tuples x the next slot's k best labels, exact).  Ties go to the candidate order: partial rank
 *   major, slot rank minor, a slot's ranks being sir_classify's.  best_index is the tuple's mixed-radix number, slot 0 most
 *   significant (< 8^8); best_prob = expf(s_t); valid_mass, if given, is 1; ranks beyond prod C_g are padded as above.
 *   A row with a NaN or an infinity in ANY segment has -1 / NaN in every output; other rows are unaffected. */
int sir_decode_slots(sir_handle* h, const float* logits, int batch, int num_classes, const int32_t* slot_sizes, int n_slots,
                     const float* inv_temperature, const uint8_t* tuples, int n_tuples, int k, int32_t* best_index,
                     int32_t* best_labels, float* best_logp, float* best_prob, float* valid_mass, float* tuple_logp, void* stream);

/* ---- embeddings and the prototype head (DESIGN.md section 4 "Embeddings and the prototype head", csrc/prototypes.hip) -------
 * Intents enrolled from examples, with no backward pass: the unit-normalised embeddings (sir_model_embed) of a class's examples
 * are summed into a bank, the normalised sums are the class prototypes, and a batch is scored by cosine similarity against up
 * to 4096 prototypes or exemplars in one launch.  Nothing allocates; no floating-point atomics; results bit-reproducible.
 * Embedding rows are [512] f32, arrays of them 16-byte aligned.  The UNIT VECTOR of a row e is u = e / ||e|| with the norm and
 * the quotient in double; the row's sum of squares is taken in a fixed order that depends on nothing but the row (element
 * 8 l + i in lane l: the lane's eight squares in order i, then the xor butterfly over the lanes).  Every argument is checked
 * before anything is launched; a refused call (SIR_EINVAL: a required pointer NULL, a count outside its range, k > 8, a
 * misaligned pointer, state_bytes too small, the header's n_classes different from the argument) writes nothing.
 *
 * The bank is caller-owned DEVICE memory of sir_proto_state_bytes(n_classes) bytes (0 unless 1 <= n_classes <= 4096), 16-byte
 * aligned, P = n_classes:
 *     bytes 0..63   header: int32 n_classes, int32 0, int64 skipped, zeros
 *     int64  count[P]
 *     double sum[P][512]
 * sir_proto_reset lays the state out: it clears count and sum of the classes with mask[p] != 0 (mask: DEVICE uint8[P]; NULL =
 *   all, which also zeroes `skipped` and needs no valid header).  A class is removed or re-enrolled this way.
 * sir_proto_accumulate: for each row b in ascending order, sum[labels[b]] += u_b (double), count[labels[b]] += 1.  labels:
 *   DEVICE int64[batch].  A class's sum is ONE sequential chain in row order (one wavefront per class walks the labels), so THE
 *   STATE AFTER ENROLLING A SET OF ROWS IS BIT-IDENTICAL HOWEVER THE ROWS WERE CUT INTO CALLS.  A row is skipped, counted in
 *   `skipped` and leaves everything else untouched when its label is outside [0, n_classes) (-1 is the documented "ignore"), its
 *   embedding holds a NaN or an infinity, or its norm is zero.  The norm being a double, a finite row at 1e-30 or 1e30 enrols
 *   like any other.
 * sir_proto_finalize: protos[p] = fp32(sum[p] / ||sum[p]||) in double, live[p] = 1; a class with count 0 or a zero or
 *   non-finite sum gets an all-zero row and live[p] = 0.  protos [P][512] f32, live uint8[P], both required.
 * sir_proto_accumulate, sir_proto_finalize and a masked sir_proto_reset read the header back before they launch: they are
 * host-synchronous on `stream` and not legal under stream capture.  Calls on one state must be ordered (one stream, or events). */
size_t sir_proto_state_bytes(int n_classes);
int sir_proto_reset(sir_handle* h, void* state, size_t state_bytes, int n_classes, const uint8_t* mask /* NULL: all */, void* stream);
int sir_proto_accumulate(sir_handle* h, void* state, size_t state_bytes, int n_classes, const float* emb, const int64_t* labels,
                         int batch, void* stream);
int sir_proto_finalize(sir_handle* h, void* state, size_t state_bytes, int n_classes, float* protos, uint8_t* live, void* stream);
/* sir_proto_score: one launch, only a kernel (legal under stream capture).  1 <= batch <= 2^30, 1 <= n_protos <= 4096,
 * 1 <= n_classes <= n_protos, 1 <= k <= 8.
 *   protos      f32 [n_protos][512]: unit rows (sir_proto_finalize's, or exemplars); finite
 *   live        DEVICE uint8[n_protos] or NULL (all live)
 *   proto_class DEVICE int32[n_protos], the class of each prototype, or NULL: class = row, and n_classes must equal n_protos.
 *               A prototype whose class is outside [0, n_classes) takes no part, like one that is not live.
 *   scale       DEVICE f32[1] or NULL = 1: used as given, the way sir_classify uses inv_temperature -- the ranking never
 *               depends on it; a value that is not positive and finite gives the probabilities IEEE arithmetic gives.
 * Per row: u = the unit vector of emb[b]; sim[p] = <u, protos[p]> in fp32 (an fma chain over the lane's eight elements, then a
 * fixed butterfly over the lanes); the score of class c is s[c] = max of sim[p] over its live prototypes (one per class: a
 * nearest-class-mean head; several exemplars: 1-NN); a class with no live prototype is absent.  Classes rank by descending s,
 * equal scores by ascending class, as sir_classify.
 *   sims        f32 [batch][n_protos] or NULL: every sim[p], live or not
 *   topk_class  int32 [batch][k], topk_sim f32 [batch][k] = s, topk_prob f32 [batch][k] = the softmax of scale * s over the
 *               present classes: expf((s - max s) * scale) / den, den summed in double in a fixed order
 *   nearest     int32 [batch] or NULL: the lowest live prototype row of the rank-0 class whose sim is that class's score
 * Ranks beyond the number of present classes hold -1 / 0 / 0 (nearest -1 with no class present).  A row of emb that holds a
 * NaN or an infinity or has norm zero gives -1 / NaN / NaN, nearest -1 and NaN sims; the other rows are unaffected.
 * A ROW'S OUTPUTS CARRY THE SAME BITS WHATEVER ITS POSITION IN THE BATCH AND WHATEVER THE BATCH SIZE. */
int sir_proto_score(sir_handle* h, const float* emb, int batch, const float* protos, const uint8_t* live /* or NULL */,
                    const int32_t* proto_class /* or NULL: class = row */, int n_protos, int n_classes,
                    const float* scale /* device scalar or NULL = 1 */, int k, float* sims /* or NULL */, int32_t* topk_class,
                    float* topk_sim, float* topk_prob, int32_t* nearest /* or NULL */, void* stream);

/* ---- training the embedding: the cosine-proxy loss ------------------------------------------------
 * A normalised-softmax (AM-softmax / CosFace-style) loss of the embeddings against one learned centre per class, and its
 * gradients.  With u_b = emb[b] / ||emb[b]|| and q_k = proxies[k] / ||proxies[k]|| (norms and quotients in double, the code of
 * sir_proto_score; the unit vectors rounded to fp32 as there):
 *     z[b][k] = scale * (<u_b, q_k> - margin * [k == labels[b]])       (the dot product of sir_proto_score, the same bits)
 *     loss    = mean over the rows with a label of -log softmax(z[b])[labels[b]]
 *     dz      = (softmax - onehot) * grad_scale / n_valid
 *     demb[b]     = (du - <du, u_b> u_b) / ||emb[b]||,     du = scale * sum_k dz[b][k] q_k
 *     dproxies[k] = (dq - <dq, q_k> q_k) / ||proxies[k]||, dq = scale * sum_b dz[b][k] u_b
 * 1 <= batch, 1 <= n_proxies <= 4096 (the bank's limit); scale > 0 and margin >= 0 are HOST floats, finite.
 *   emb      f32 [batch][512], proxies f32 [n_proxies][512] (need not be unit), labels DEVICE int64[batch]
 *   loss     DEVICE f32[1]; demb f32 [batch][512] or NULL; dproxies f32 [n_proxies][512] or NULL (written, not accumulated)
 *   workspace  sir_proxy_loss_workspace_bytes(batch, n_proxies) bytes (0 for counts outside the limits), 16-byte aligned
 * Labels as for sir_ce_loss: -100 takes the row out of the loss, the gradients (a zero demb row) and the divisor (every row
 * ignored: 0 / 0 = NaN); any other label outside [0, n_proxies) makes the loss NaN, gives the row no gradient and raises the
 * status bit of sir_ce_loss (SIR_EINVAL at the next sir_check_status).  A row of emb or proxies with a NaN, an infinity or norm
 * zero has no direction: the loss and that row's gradients are NaN, unless the row of emb is ignored.
 * No floating atomic and every sum in a fixed order: bit-reproducible, and a row's demb carries the same bits at any position and
 * batch size for equal n_valid.  Only kernels, no allocation: legal under stream capture.  Every argument is validated before
 * anything is launched; a refused call (SIR_EINVAL) writes nothing.  These launches carry no profile ids. */
size_t sir_proxy_loss_workspace_bytes(int batch, int n_proxies);
int sir_proxy_loss(sir_handle* h, const float* emb, const float* proxies, const int64_t* labels, int batch, int n_proxies,
                   float scale, float margin, float* loss, float* demb /* or NULL */, float* dproxies /* or NULL */,
                   float grad_scale, void* workspace, size_t workspace_bytes, void* stream);

/* ---- measurement -----------------------------------------------------------------------------
 * HIP-event timing of the kernels of the path, recorded on the stream they are launched on
 * (bench.py's roofline figures come from here).  mode 0 = off, 1 = every kernel, 2 = only
 * `kernel_id`.  sir_profile_collect waits for the recorded events, returns per-kernel total
 * milliseconds and launch counts since the last collect (arrays of length n), and resets. */
/* Extended ids: kernels of optional calls are numbered BEHIND sir_profile_kernel_count(), so that a caller walking
 * [0, sir_profile_kernel_count()) sees the list it always saw.  sir_profile_kernel_name, sir_profile_enable and
 * sir_profile_collect (n up to count + SIR_PROFILE_EXTRA_IDS) serve them:
 *   count + 0  "bwd_conv1_dgrad"   conv1's data gradient (sir_model_train_bwd_x with dfeats) */
#define SIR_PROFILE_EXTRA_IDS 1
int sir_profile_kernel_count(void);
const char* sir_profile_kernel_name(int kernel_id);
int sir_profile_enable(sir_handle* h, int mode, int kernel_id);
int sir_profile_collect(sir_handle* h, double* total_ms, int64_t* launches, int n);

#ifdef __cplusplus
}
#endif
#endif /* SIR_HIP_H */
