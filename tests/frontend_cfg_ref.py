"""Reference of the feature path at any front-end (n_fft, hop_length, win_length), written from torchaudio's documented arithmetic:

  MelSpectrogram(sample_rate, n_fft, win_length, hop_length, n_mels)   torch.stft(center=True, pad_mode="reflect", periodic Hann of
      win_length centred in the frame), power 2, HTK filterbank (norm None, f_min 0, f_max sample_rate // 2)
  AmplitudeToDB()                                                      10 log10(max(x, 1e-10))
  whole-utterance z-norm                                               (x - mean) / (unbiased std + 1e-5), before any trim
  pad / trim to t_pad frames

``*_f32`` runs torch.stft in float32 (what the reference's CPU path would execute), ``*_f64`` is numpy float64 from first principles
(np.fft.rfft over explicitly padded frames).  oracle/features_ref.py is the same pair fixed at 1024 / 512 / 1024.
The filterbank is torchaudio's float32 TABLE in both (``htk_mel_fbanks``: melscale_fbanks computes it in float32, and the kernel is
handed that table bit for bit), promoted to double in ``*_f64``: the table is an input of the arithmetic, and its own float32
rounding against ``mel_fbank_f64`` -- up to 5e-6 of a weight, which reaches 5e-4 dB on a one-bin filter of n_fft 256 -- is no
error of either implementation.
"""
import numpy as np
import torch

from sir_amd.featurizer import htk_mel_fbanks

SAMPLE_RATE = 16000
N_MELS = 64
AMIN = 1e-10
NORM_EPS = 1e-5


def num_frames(length, n_fft, hop):
    """torch.stft(center=True): 1 + L // hop frames; a clip of <= n_fft / 2 samples cannot be reflect-padded (zero row)."""
    return 1 + length // hop if length > n_fft // 2 else 0


def mel_fbank_f64(n_freqs, n_mels=N_MELS, sample_rate=SAMPLE_RATE):
    all_freqs = np.linspace(0.0, sample_rate // 2, n_freqs)
    m_max = 2595.0 * np.log10(1.0 + (sample_rate // 2) / 700.0)
    f_pts = 700.0 * (10.0 ** (np.linspace(0.0, m_max, n_mels + 2) / 2595.0) - 1.0)
    fb = np.zeros((n_freqs, n_mels))
    for j in range(n_mels):
        lo, ce, hi = f_pts[j], f_pts[j + 1], f_pts[j + 2]
        fb[:, j] = np.maximum(0.0, np.minimum((all_freqs - lo) / (ce - lo), (hi - all_freqs) / (hi - ce)))
    return fb


def features_f32(wave, n_fft, hop, win=None, n_mels=N_MELS, sample_rate=SAMPLE_RATE):
    """float32 [L] -> {"db", "norm"}: float32 [n_mels, T] tensors, or None for a clip of <= n_fft / 2 samples."""
    win = n_fft if win is None else win
    wave = torch.as_tensor(wave, dtype=torch.float32)
    if wave.numel() <= n_fft // 2:
        return None
    spec = torch.stft(wave, n_fft=n_fft, hop_length=hop, win_length=win,
                      window=torch.hann_window(win, periodic=True, dtype=torch.float32), center=True, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True).abs().pow(2.0)
    fb = htk_mel_fbanks(n_fft // 2 + 1, 0.0, float(sample_rate // 2), n_mels, sample_rate).float()
    mel = torch.matmul(spec.transpose(-1, -2), fb).transpose(-1, -2)
    db = 10.0 * torch.log10(torch.clamp(mel, min=AMIN))
    return {"db": db, "norm": (db - db.mean()) / (db.std() + NORM_EPS)}


def features_f64(wave, n_fft, hop, win=None, n_mels=N_MELS, sample_rate=SAMPLE_RATE):
    """float64 numpy twin of ``features_f32``."""
    win = n_fft if win is None else win
    x = np.asarray(wave, dtype=np.float64)
    if x.size <= n_fft // 2:
        return None
    xp = np.pad(x, (n_fft // 2, n_fft // 2), mode="reflect")
    w = np.zeros(n_fft)
    left = (n_fft - win) // 2
    w[left:left + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    t = 1 + x.size // hop
    frames = np.stack([xp[i * hop: i * hop + n_fft] * w for i in range(t)])
    spec = np.abs(np.fft.rfft(frames, axis=1)) ** 2
    fb = htk_mel_fbanks(n_fft // 2 + 1, 0.0, float(sample_rate // 2), n_mels, sample_rate).double().numpy()
    mel = (spec @ fb).T
    db = 10.0 * np.log10(np.maximum(mel, AMIN))
    return {"db": db, "norm": (db - db.mean()) / (db.std(ddof=1) + NORM_EPS)}


def pad_or_trim(feat, t_pad):
    """[n_mels, T] -> [n_mels, t_pad] (tensor or array), zeros behind the clip."""
    feat = torch.as_tensor(feat)
    if feat.shape[1] >= t_pad:
        return feat[:, :t_pad]
    return torch.nn.functional.pad(feat, (0, t_pad - feat.shape[1]))


def batch_f32(waves, n_fft, hop, win, t_pad, n_mels=N_MELS):
    """list of float32 [L_i] -> (norm [B, n_mels, t_pad], db [B, n_mels, t_pad]) float32; too-short clips are zero rows."""
    norm, db = [], []
    for w in waves:
        f = features_f32(w, n_fft, hop, win, n_mels)
        if f is None:
            norm.append(torch.zeros(n_mels, t_pad))
            db.append(torch.zeros(n_mels, t_pad))
        else:
            norm.append(pad_or_trim(f["norm"], t_pad))
            db.append(pad_or_trim(f["db"], t_pad))
    return torch.stack(norm), torch.stack(db)


def chirp_clips(n, length, seed, sample_rate=SAMPLE_RATE):
    """Linear chirp of amplitude 0.2 in white noise of sigma 0.1 (no pure tone: the dynamic range of a tone is beyond float32 FFT
    agreement; at this mix the float32 reference stays within 1e-5 of the float64 one, tests/test_frontend_cfg_host.py),
    float32 [n, length]."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(length, dtype=torch.float64) / sample_rate
    out = []
    for i in range(n):
        f0 = 200.0 + 150.0 * i
        f1 = 3000.0 + 400.0 * i
        dur = max(length / sample_rate, 1e-3)
        phase = 2.0 * np.pi * (f0 * t + 0.5 * (f1 - f0) / dur * t * t)
        x = 0.2 * torch.sin(phase) + 0.1 * torch.randn(length, generator=g, dtype=torch.float64)
        out.append(x.float())
    return torch.stack(out)
