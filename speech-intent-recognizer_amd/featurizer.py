"""Batched log-mel features on the GPU (host side of ``sir_features_fwd``).

One call turns a whole batch of waveforms resident in HBM into normalised, padded
``[B, n_mels, t_pad]`` features -- what the reference does one file at a time on the CPU in
``AudioFeatureExtractor.extract_features`` (scripts/precompute_features.py:59-73) followed by the
pad/trim of ``FSCIntentDataset.__getitem__`` (scripts/dataset.py:109-113).
"""
import ctypes as C
import math

import torch
from torch.autograd.function import once_differentiable

from . import _native, wave_args

N_FFT = 1024
HOP = 512
MAX_DURATION_S = 5.0
# what sir_features_bwd answers on a handle of another front-end (csrc/api.hip); HipFeaturizer.differentiable raises it before
# any device call
GRAD_DEFAULT_ONLY = ("sir_features_bwd: the waveform gradient is built for the default front-end only (n_fft 1024 / "
                     "hop_length 512 / win_length 1024; this handle has {} / {} / {})")


def is_default_frontend(n_fft, hop_length, win_length=None):
    """True for the front-end the specialised one-launch kernel (and the waveform gradient) is built for."""
    return (int(n_fft), int(hop_length), int(n_fft if win_length is None else win_length)) == (N_FFT, HOP, N_FFT)


def htk_mel_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate):
    """float32 filterbank [n_freqs, n_mels] with the arithmetic torchaudio's MelScale uses
    (HTK scale, norm=None), so the kernel gets the reference's own table bit for bit."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.min(down, up), min=0.0).contiguous()


def _check_wave_grad_args(wave, lengths, t_pad, hop=HOP):
    """Host-only checks of the differentiable feature path (no device call): float32 ``[B, L]`` on the GPU, one length per
    clip, and every frame of the longest clip inside ``t_pad`` (the z-norm statistics run over all of them)."""
    if not torch.is_tensor(wave) or wave.dtype != torch.float32:
        raise _native.SirError("the differentiable feature path takes a float32 waveform (an int16 tensor cannot carry a "
                               "gradient; dequantise it first: wave.float() / 32768)")
    if not wave_args.is_batch_layout(wave) or wave.numel() == 0:
        raise _native.SirError(f"wave must be [B, L] with unit inner stride, got {tuple(wave.shape)}")
    if lengths is not None and not wave_args.is_length_vector(lengths, wave.shape[0]):
        raise _native.SirError(f"lengths must be an integer tensor with one sample count per clip (batch {wave.shape[0]})")
    t_pad = int(t_pad)
    if t_pad < 1 or 1 + wave.shape[1] // hop > t_pad:
        raise _native.SirError(f"clips of {wave.shape[1]} samples have {1 + wave.shape[1] // hop} frames: the gradient needs "
                               f"t_pad >= that (got {t_pad})")
    if not wave.is_cuda or (lengths is not None and not lengths.is_cuda):
        raise _native.SirError("tensor is not on a HIP device: this path runs on MI355X only (no CPU fallback)")


REVERB_KEYS = ("rir", "noise", "rir_index", "noise_index", "noise_offset", "snr_db")


def reject_reverb_args(kw, who):
    """The differentiable forms stop at the feature extractor: the gradient through ``sir_wave_reverb_mix`` does not exist."""
    given = sorted(k for k in REVERB_KEYS if kw.get(k) is not None)
    if given:
        raise ValueError(f"{who} does not take reverb / background-noise arguments ({', '.join(given)}): the gradient through "
                         "the convolution is not implemented; apply HipFeaturizer.reverb_mix first and differentiate from there")
    unknown = sorted(k for k in kw if k not in REVERB_KEYS)
    if unknown:
        raise TypeError(f"{who} got unexpected keyword arguments: {', '.join(unknown)}")


class _DifferentiableFeatures(torch.autograd.Function):
    """``sir_features_fwd`` (keeping its dB tile) / ``sir_features_bwd``."""

    @staticmethod
    def forward(ctx, wave, fz, lengths, t_pad, aug):
        db = torch.empty((wave.shape[0], fz.n_mels, t_pad), dtype=torch.float32, device=wave.device)
        out = fz(wave, lengths, t_pad=t_pad, db_out=db, **aug)
        ctx.fz, ctx.wave, ctx.lengths, ctx.t_pad, ctx.aug, ctx.db = fz, wave, lengths, t_pad, aug, db
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        dwave = ctx.fz.features_bwd(ctx.wave, ctx.lengths, ctx.db, dout, t_pad=ctx.t_pad, **ctx.aug)
        return dwave, None, None, None, None


class HipFeaturizer:
    """Owns one ``sir_handle`` on the current HIP device."""

    def __init__(self, sample_rate=16000, n_mels=64, n_fft=N_FFT, hop_length=HOP, win_length=None):
        _native.require_hip()
        win_length = int(n_fft if win_length is None else win_length)
        self.sample_rate, self.n_mels, self.n_fft, self.hop_length = sample_rate, n_mels, n_fft, hop_length
        self.win_length = win_length
        self.device = torch.device("cuda", torch.cuda.current_device())
        # (sir_create_ex rejects an unsupported front-end before it reads the window)
        window = torch.hann_window(max(win_length, 1), periodic=True, dtype=torch.float32).contiguous()
        fb = htk_mel_fbanks(n_fft // 2 + 1, 0.0, float(sample_rate // 2), n_mels, sample_rate).float().contiguous()
        cfg = _native.FeatureConfig(sample_rate, n_fft, hop_length, n_mels, 0.0, float(sample_rate // 2),
                                    window.data_ptr(), fb.data_ptr())
        self._h = C.c_void_p()
        _native.check(_native.lib().sir_create_ex(C.byref(cfg), win_length, C.byref(self._h)), "sir_create_ex")
        self._scratch = wave_args.StreamScratch()      # workspaces of __call__, perturb and reverb_mix, one per calling stream
        self._pins = 0          # library objects (sir_pipeline) created from this handle that are still alive

    def pin(self):
        """Called by whoever creates a longer-lived library object from this handle (``sir_pipeline``, kept for the life of
        the process: sir_amd/pipeline.py): the handle must then outlive it, so ``__del__`` leaves it to process exit."""
        self._pins += 1

    def __del__(self):
        try:
            if getattr(self, "_pins", 0) > 0:
                return
            if getattr(self, "_h", None):
                _native.lib().sir_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def num_frames(self, length):
        return 1 + length // self.hop_length

    def __call__(self, wave, lengths=None, t_pad=200, shift=None, noise_sigma=None, noise_seed=0,
                 time_mask=None, freq_mask=None, out=None, db_out=None):
        """wave: [B, L] float32 or int16 on the GPU; lengths: int32 [B] on the GPU (default: all L).
        ``db_out`` (optional, same shape as the result) receives the un-normalised dB values.
        Returns [B, n_mels, t_pad] float32."""
        dt, bsz, max_len, lengths = wave_args.check_batch("features", wave, lengths)
        if out is None:
            out = torch.empty((bsz, self.n_mels, t_pad), dtype=torch.float32, device=wave.device)
        lib = _native.lib()
        ws = self._scratch.get(lib.sir_features_workspace_bytes(self._h, bsz, max_len), wave.device)
        keep = wave_args.Keep(wave.device)
        rc = lib.sir_features_fwd(self._h, wave.data_ptr(), dt, wave.stride(0), lengths.data_ptr(), bsz, max_len,
                                  out.data_ptr(), t_pad, db_out.data_ptr() if db_out is not None else None,
                                  ws.data_ptr(), ws.numel(),
                                  keep.augment(shift, noise_sigma, noise_seed, time_mask, freq_mask), _native.current_stream_ptr())
        _native.check(rc, "sir_features_fwd")
        return out

    def differentiable(self, wave, lengths=None, t_pad=200, shift=None, noise_sigma=None, noise_seed=0,
                       time_mask=None, freq_mask=None, **reverb_kw):
        """``__call__`` as a node of the autograd graph: the same ``[B, n_mels, t_pad]`` features (the same launch), and
        ``wave.grad`` after a backward (``sir_features_bwd``; DESIGN.md "Gradients down to the waveform").  ``wave`` must be
        float32 ``[B, L]`` with ``1 + L // hop <= t_pad``; once differentiable (a double backward raises).  The noise of
        ``noise_sigma`` is regenerated from ``noise_seed`` in the backward; masked outputs pass no gradient.  The arguments of
        ``reverb_mix`` are rejected with ``ValueError`` (no gradient through the convolution)."""
        reject_reverb_args(reverb_kw, "HipFeaturizer.differentiable")
        n_fft = getattr(self, "n_fft", N_FFT)
        win_length = getattr(self, "win_length", n_fft)
        if not is_default_frontend(n_fft, self.hop_length, win_length):
            raise _native.SirError(GRAD_DEFAULT_ONLY.format(n_fft, self.hop_length, win_length))
        _check_wave_grad_args(wave, lengths, t_pad, self.hop_length)
        if lengths is not None:
            lengths = lengths.to(torch.int32).contiguous()
        aug = dict(shift=shift, noise_sigma=noise_sigma, noise_seed=noise_seed, time_mask=time_mask, freq_mask=freq_mask)
        return _DifferentiableFeatures.apply(wave, self, lengths, int(t_pad), aug)

    def features_bwd(self, wave, lengths, db, dout, t_pad=200, shift=None, noise_sigma=None, noise_seed=0,
                     time_mask=None, freq_mask=None, out=None):
        """``sir_features_bwd``: d loss / d wave ``[B, L]`` float32 from ``dout = d loss / d features`` and the ``db_out`` of the
        matching ``__call__`` (same wave -- float32 or int16 --, lengths, t_pad and augmentation arguments).  ``out``
        (optional): float32 ``[B, >= L]`` with unit inner stride; columns from L on are left alone."""
        dt, bsz, max_len, lengths = wave_args.check_batch("features_bwd", wave, lengths)
        _native.require_hip(db, dout)
        shape = (bsz, self.n_mels, int(t_pad))
        for name, t in (("db", db), ("dout", dout)):
            if t.dtype != torch.float32 or tuple(t.shape) != shape:
                raise _native.SirError(f"{name} must be float32 {shape}, got {t.dtype} {tuple(t.shape)}")
        db, dout = db.contiguous(), dout.contiguous()
        out = wave_args.check_out(out, bsz, max_len, wave.device)
        keep = wave_args.Keep(wave.device)
        rc = _native.lib().sir_features_bwd(self._h, wave.data_ptr(), dt, wave.stride(0), lengths.data_ptr(), bsz, max_len,
                                            db.data_ptr(), dout.data_ptr(), int(t_pad),
                                            keep.augment(shift, noise_sigma, noise_seed, time_mask, freq_mask), out.data_ptr(),
                                            wave_args.out_row_stride(out), _native.current_stream_ptr())
        _native.check(rc, "sir_features_bwd")
        return wave_args.first_cols(out, max_len)

    # ---- waveform front-end (channel mix-down, sample-rate conversion) -----------------------------
    def mix_to_mono(self, pcm, channels, frames=None):
        """pcm: [B, frames * channels] interleaved int16 or float32 on the GPU -> [B, frames] float32
        (``torch.mean(waveform, dim=0)`` of precompute_features.py:50-51 after torchaudio.load's /32768)."""
        _native.require_hip(pcm, frames)
        must = "pcm must be [B, frames * channels]"
        dt, bsz, width = wave_args.check_wave("mix_to_mono", pcm, must, kind="sample")
        if width % channels:
            raise _native.SirError(f"mix_to_mono: {must} with unit inner stride")
        max_frames = width // channels
        if frames is not None:
            frames = wave_args.check_lengths("mix_to_mono", frames, bsz)
        out = torch.empty((bsz, max_frames), dtype=torch.float32, device=pcm.device)
        rc = _native.lib().sir_mix_to_mono(self._h, pcm.data_ptr(), dt, channels, pcm.stride(0),
                                           frames.data_ptr() if frames is not None else None, bsz, max_frames,
                                           out.data_ptr(), out.stride(0), _native.current_stream_ptr())
        _native.check(rc, "sir_mix_to_mono")
        return out

    def resample(self, wave, orig_freq, new_freq=None, lengths=None):
        """``torchaudio.transforms.Resample(orig_freq, new_freq)`` (precompute_features.py:54-56) for a batch:
        wave [B, L] float32/int16 on the GPU, lengths int32 [B] -> ([B, ceil(new * L / orig)] float32, out lengths)."""
        new_freq = self.sample_rate if new_freq is None else new_freq
        dt, bsz, max_len, lengths = wave_args.check_batch("resample", wave, lengths)
        if int(orig_freq) == int(new_freq):
            return (wave if wave.dtype == torch.float32 else wave.float() / 32768.0), lengths
        lib = _native.lib()
        max_out = lib.sir_resample_out_len(max_len, int(orig_freq), int(new_freq))
        if max_out < 0:
            raise _native.SirError(f"resample: bad rates {orig_freq} -> {new_freq} Hz, or the output of {max_len} samples "
                                   "does not fit an int32 length")
        out = torch.empty((bsz, max_out), dtype=torch.float32, device=wave.device)
        out_len = torch.empty((bsz,), dtype=torch.int32, device=wave.device)
        rc = lib.sir_resample(self._h, wave.data_ptr(), dt, wave.stride(0), lengths.data_ptr(), bsz, max_len,
                              int(orig_freq), int(new_freq), out.data_ptr(), out.stride(0), max_out,
                              out_len.data_ptr(), _native.current_stream_ptr())
        _native.check(rc, "sir_resample")
        return out, out_len

    # ---- pitch / tempo perturbation (scripts/augment.py:30-80 pitch_shift / speed_change) -------------------------
    def perturb(self, wave, lengths=None, shift=None, pitch_cents=None, tempo=None, max_out_len=None, offsets_out=None):
        """Per-utterance shift -> pitch -> speed (``sir_wave_perturb``) of a GPU batch: wave [B, L]
        float32/int16, lengths int32 [B] (default all L); ``shift`` int32 [B] samples, ``pitch_cents`` float32 [B] in
        [-200, 200] (0 = not drawn), ``tempo`` float32 [B] in [0.5, 2] (1 = not drawn), each optional (None = off).
        ``max_out_len`` defaults to the longest output of the reference's tempo range (L at tempo 0.85; rows of a slower
        tempo are cut there).
        ``offsets_out`` (test hook): int32 [B, 2, max_segments] receives the chosen WSOLA offsets, -1 where unused.
        Returns (out [B, max_out_len] float32, zero beyond each row's length, out_lengths int32 [B])."""
        _native.require_hip(offsets_out)
        dt, bsz, max_len, lengths = wave_args.check_batch("perturb", wave, lengths, refuse_empty=True)
        lib = _native.lib()
        keep = wave_args.Keep(wave.device, bsz)
        p_shift = keep.ptr(shift, torch.int32)
        p_cents, p_tempo = keep.ptr(pitch_cents, torch.float32), keep.ptr(tempo, torch.float32)
        if max_out_len is None:
            max_out_len = lib.sir_perturb_out_len(max_len, 0.85) if tempo is not None else max_len
            max_out_len = max(max_out_len, max_len)
        max_out_len = int(max_out_len)
        out = torch.empty((bsz, max_out_len), dtype=torch.float32, device=wave.device)
        out_len = torch.empty((bsz,), dtype=torch.int32, device=wave.device)
        ws, nbytes = None, 0
        if pitch_cents is not None:
            buf = self._scratch.get(lib.sir_perturb_workspace_bytes(self._h, bsz, max_len), wave.device)
            ws, nbytes = buf.data_ptr(), buf.numel()
        max_seg = 0
        if offsets_out is not None:
            if offsets_out.dtype != torch.int32 or not offsets_out.is_contiguous() or offsets_out.dim() != 3 \
                    or tuple(offsets_out.shape[:2]) != (bsz, 2):
                raise _native.SirError("offsets_out must be a contiguous int32 [B, 2, max_segments] tensor")
            max_seg = offsets_out.shape[2]
        rc = lib.sir_wave_perturb(self._h, wave.data_ptr(), dt, wave.stride(0), lengths.data_ptr(), bsz, max_len,
                                  p_shift, p_cents, p_tempo, out.data_ptr(), out.stride(0), max_out_len, out_len.data_ptr(),
                                  offsets_out.data_ptr() if offsets_out is not None else None, max_seg, ws, nbytes,
                                  _native.current_stream_ptr())
        _native.check(rc, "sir_wave_perturb")
        return out, out_len

    # ---- room reverberation and background noise at a chosen SNR (sir_wave_reverb_mix) -----------------------------
    def reverb_mix(self, wave, lengths=None, rir=None, noise=None, rir_index=None, noise_index=None, noise_offset=None,
                   snr_db=None, out=None, return_gain=False):
        """Per-utterance reverb -> background noise (``sir_wave_reverb_mix``) of a GPU batch: wave [B, L]
        float32/int16, lengths int32 [B] (default all L).  ``rir`` / ``noise``: ``SoundBank``s (sir_amd/sound_bank.py);
        ``rir_index`` / ``noise_index`` int32 [B] rows of them, -1 = not drawn for that clip (None = effect off);
        ``noise_offset`` int32 [B] first noise sample (the noise wraps), ``snr_db`` float32 [B].  A clip keeps its length.
        ``out`` (optional): float32 [B, >= L] with unit inner stride, not overlapping ``wave``; columns from L on are left alone.
        Returns out [B, L] float32, zero beyond each row's length (``return_gain``: also the gain applied to each row's noise)."""
        dt, bsz, max_len, lengths = wave_args.check_batch("reverb_mix", wave, lengths, refuse_empty=True)
        if (rir_index is not None and rir is None) or (noise_index is not None and noise is None):
            raise _native.SirError("rir_index / noise_index need their SoundBank (rir= / noise=)")
        if noise_index is not None and (noise_offset is None or snr_db is None):
            raise _native.SirError("noise_index needs noise_offset and snr_db")
        lib = _native.lib()
        keep = wave_args.Keep(wave.device, bsz)

        def bank(b, on):
            if not on:
                return None, 0, None, 0, 0
            b = b.on(wave.device)
            keep.held.append(b)
            return b.data.data_ptr(), b.data.stride(0), b.lengths.data_ptr(), len(b), b.max_len
        p_ri, p_ni = keep.ptr(rir_index, torch.int32), keep.ptr(noise_index, torch.int32)
        p_off, p_snr = None, None
        if noise_index is not None:
            p_off, p_snr = keep.ptr(noise_offset, torch.int32), keep.ptr(snr_db, torch.float32)
        r_data, r_stride, r_len, n_rir, max_rir = bank(rir, rir_index is not None)
        n_data, n_stride, n_len, n_noise, _ = bank(noise, noise_index is not None)
        out = wave_args.check_out(out, bsz, max_len, wave.device)
        ws = self._scratch.get(lib.sir_reverb_workspace_bytes(self._h, bsz, max_len, max_rir), wave.device)
        rc = lib.sir_wave_reverb_mix(self._h, wave.data_ptr(), dt, wave.stride(0), lengths.data_ptr(), bsz, max_len,
                                     r_data, r_stride, r_len, n_rir, max_rir, p_ri,
                                     n_data, n_stride, n_len, n_noise, p_ni, p_off, p_snr,
                                     out.data_ptr(), wave_args.out_row_stride(out),
                                     ws.data_ptr(), ws.numel(), _native.current_stream_ptr())
        _native.check(rc, "sir_wave_reverb_mix")
        res = wave_args.first_cols(out, max_len)
        if return_gain:
            return res, ws[:bsz * 4].view(torch.float32).clone()
        return res


_featurizers = {}


def get_featurizer(sample_rate=16000, n_mels=64, n_fft=N_FFT, hop_length=HOP, win_length=None):
    """Per-device cached featurizer (``win_length`` None = ``n_fft``)."""
    _native.require_hip()
    win_length = int(n_fft if win_length is None else win_length)
    key = (torch.cuda.current_device(), sample_rate, n_mels, n_fft, hop_length, win_length)
    if key not in _featurizers:
        _featurizers[key] = HipFeaturizer(sample_rate, n_mels, n_fft, hop_length, win_length)
    return _featurizers[key]
