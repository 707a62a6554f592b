"""The feature path restated in differentiable torch float64 -- the reference of ``sir_features_bwd``.

Step by step what ``oracle.features_ref.extract_features_f64`` does in numpy (reflect pad, frames, periodic Hann, ``rfft``, the
float64 HTK filterbank of ``oracle.features_ref.mel_fbank_f64``, 1e-10 clamp, dB, whole-utterance unbiased z-norm), plus what
``sir_features_fwd`` adds around it: the time shift and the additive noise in front, the SpecAugment bands and the zero padding to
``t_pad`` behind.  The gradient is taken by autograd.  Two rules are explicit, as in include/sir_hip.h: a mel value at or below the
clamp passes no gradient, and a constant dB tile (sigma == 0) is normalised by the constant 1e-5.
"""
import numpy as np
import torch

from oracle import features_ref

N_FFT, HOP, AMIN, NORM_EPS = features_ref.N_FFT, features_ref.HOP, features_ref.AMIN, features_ref.NORM_EPS
_FB = torch.from_numpy(features_ref.mel_fbank_f64())                    # [513, 64] float64
_N = torch.arange(N_FFT, dtype=torch.float64)
_WIN = 0.5 - 0.5 * torch.cos(2.0 * np.pi * _N / N_FFT)


def shifted(x, shift):
    """``time_shift``: > 0 delays (zero fill on the left), < 0 advances; same length."""
    if shift == 0:
        return x
    z = torch.zeros(abs(shift), dtype=x.dtype)
    return torch.cat([z, x[: x.numel() - shift]]) if shift > 0 else torch.cat([x[-shift:], z])


def features_f64(x, t_pad=None, shift=0, noise=None, time_mask=None, freq_mask=None):
    """x: float64 [L] (L > 512) -> normalised [64, T], or [64, t_pad] with the bands zeroed when ``t_pad`` is given."""
    x = shifted(x, shift)
    if noise is not None:
        x = x + noise
    xp = torch.nn.functional.pad(x[None, None], (N_FFT // 2, N_FFT // 2), mode="reflect")[0, 0]
    return features_from_padded_f64(xp, t_pad, time_mask, freq_mask)


def features_from_padded_f64(xp, t_pad=None, time_mask=None, freq_mask=None):
    """``features_f64`` from the reflect-padded clip on (float64 [L + 1024]): differentiated with respect to ``xp`` it tells what
    each padded position contributes before the padding folds it back onto a sample."""
    frames = xp.unfold(0, N_FFT, HOP) * _WIN                             # [T, 1024]
    spec = torch.fft.rfft(frames, dim=1)
    mel = (spec.real ** 2 + spec.imag ** 2) @ _FB                        # [T, 64]
    mel = torch.where(mel > AMIN, mel, torch.full_like(mel, AMIN))       # (no gradient at or below the clamp)
    db = (10.0 * torch.log10(mel)).T                                     # [64, T]
    c = db - db.mean()
    var = (c * c).sum() / (c.numel() - 1)
    norm = c / NORM_EPS if var.item() == 0.0 else c / (var.sqrt() + NORM_EPS)
    if t_pad is None:
        return norm
    keep = torch.ones_like(norm)
    if time_mask is not None:
        keep[:, time_mask[0]: time_mask[0] + time_mask[1]] = 0.0
    if freq_mask is not None:
        keep[freq_mask[0]: freq_mask[0] + freq_mask[1], :] = 0.0
    norm = norm * keep
    t = norm.shape[1]
    return norm[:, :t_pad] if t >= t_pad else torch.nn.functional.pad(norm, (0, t_pad - t))


def grad_f64(x, dout, **kw):
    """d sum(features * dout) / d x in float64; x [L] (any float dtype), dout [64, t_pad]."""
    leaf = x.detach().double().requires_grad_(True)
    out = features_f64(leaf, t_pad=dout.shape[1], **kw)
    (g,) = torch.autograd.grad((out * dout.double()).sum(), leaf)
    return g


def grad_f32(x, dout, shift=0, noise=None, time_mask=None, freq_mask=None):
    """The same gradient through ``oracle.features_ref.extract_features_f32`` (``torch.stft`` in float32) by autograd: the
    yardstick that says what float32 arithmetic costs on this clip."""
    leaf = x.detach().float().requires_grad_(True)
    xa = shifted(leaf, shift)
    if noise is not None:
        xa = xa + noise.float()
    norm = features_ref.extract_features_f32(xa, max_duration=1e3)       # [64, T]
    t = norm.shape[1]
    g = dout.float()[:, :t].clone()
    if time_mask is not None:
        g[:, time_mask[0]: time_mask[0] + time_mask[1]] = 0.0
    if freq_mask is not None:
        g[freq_mask[0]: freq_mask[0] + freq_mask[1], :] = 0.0
    (gx,) = torch.autograd.grad((norm * g).sum(), leaf)
    return gx


def clip_error(a, ref64):
    """max |a - ref| / rms(ref) over the clip's samples."""
    ref64 = ref64.double()
    return ((a.double() - ref64).abs().max() / ref64.pow(2).mean().sqrt()).item()


def tones_and_noise(n, seed):
    """Deterministic test clip: two tones at amplitude 0.1 plus white noise (no mel value near the 1e-10 clamp)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / features_ref.SAMPLE_RATE
    f1, f2 = 300.0 + 37.0 * (seed % 11), 2100.0 + 91.0 * (seed % 7)
    x = 0.1 * torch.sin(2 * np.pi * f1 * t) + 0.1 * torch.sin(2 * np.pi * f2 * t + 0.5)
    return (x + 0.02 * torch.randn(n, generator=g, dtype=torch.float64)).float()
