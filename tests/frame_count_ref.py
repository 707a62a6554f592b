"""Inputs and CPU references of the frame-count sweep (tests/test_frame_count_host.py, tests/test_frame_count_gpu.py).

``feat_utt_kernel`` and ``feat_utt_bwd_kernel`` take all their control flow from the clip's frame count T = 1 + L // 512 and from
where L sits inside its hop; the general front ends from T alone (tiles of 64 frames, rounds of 16).  The sweeps below walk T,
and for each T the ends of its hop:

* forward: every T in 2 .. 176 (11 rounds, across the 160 / 161 switch from the register tile to parked dB values), three lengths
  each -- the first of the hop, the last, and one in between whose parity alternates from T to T + 1;
* backward: every T in 2 .. 49 (three rounds, two carries) and the neighbours of 64, 96, 128, 160 and 176, the first and the last
  length of the hop each;
* augmentation: the backward lengths at T = 2, 16, 17, 33, 160 and 161, five time shifts each (the clip shifted out but for one
  sample either way, one sample short of a hop, one past it, an odd one), noise, a time mask across the clip's end, a freq mask
  across mel 64;
* general front ends: every frame count from the smallest the handle allows to 130, one length each.

Signals: ``features_grad_ref.tones_and_noise`` (dB range -22 .. +30, nothing near the 1e-10 clamp) and, on the general front ends,
``frontend_cfg_ref.chirp_clips``.  The int16 form of a clip is ``round(x * 32767)``; the kernel reads it as ``q / 32768``, and that
float32 clip is what its reference is computed from.  Every reference is computed once per process (``lru_cache``) and must not be
written to.
"""
import functools

import numpy as np
import torch

import features_grad_ref as gref
import frontend_cfg_ref as cref
import host_rng
from oracle import features_ref

HOP = 512
T_PAD = 176
FWD_T = list(range(2, 177))
BWD_T = list(range(2, 50)) + [63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 162, 175, 176]
AUG_T = [2, 16, 17, 33, 160, 161]
GEN_CFGS = [(512, 160, 400), (256, 64, 256), (1024, 256, 1024)]
GEN_TMAX = 130
GEN_T_PAD = 132
AUG_SIGMA, AUG_SEED = 5e-3, 4242
AUG_FREQ_MASK = (60, 10)
LONG = 1e9                        # max_duration of the oracle calls: the sweep passes the reference's 5 s cut on purpose


def first_len(t):
    return max(HOP * (t - 1), HOP + 1)            # (T = 2 starts at 513: a clip of 512 samples has no frames)


def last_len(t):
    return HOP * t - 1


def mid_len(t):
    """Inside the hop, away from both ends; odd for odd T, even for even T."""
    return HOP * (t - 1) + 2 * (1 + (37 * t) % 250) + (t & 1)


def fwd_cases():
    """[(T, L)], three per frame count."""
    return [(t, n) for t in FWD_T for n in (first_len(t), mid_len(t), last_len(t))]


def bwd_cases():
    return [(t, n) for t in BWD_T for n in (first_len(t), last_len(t))]


def aug_cases():
    """[(T, L, shift)]"""
    out = []
    for t in AUG_T:
        for n in (first_len(t), last_len(t)):
            out += [(t, n, s) for s in (n - 1, -(n - 1), 511, -513, 77 + 2 * t)]
    return out


def gen_min_frames(n_fft, hop):
    return 1 + (n_fft // 2 + 1) // hop            # the shortest clip that can be reflect-padded has n_fft / 2 + 1 samples


def gen_cases(cfg):
    n_fft, hop, _ = cfg
    return [(t, max(hop * (t - 1) + (37 * t) % hop, n_fft // 2 + 1)) for t in range(gen_min_frames(n_fft, hop), GEN_TMAX + 1)]


def clip(t, n):
    """The clip of T frames and n samples; one seed per frame count (the lengths of a hop share their tones)."""
    return gref.tones_and_noise(n, seed=1000 + t)


def quantise(x):
    return (x * 32767.0).round().to(torch.int16)


def dequantise(q):
    return q.float() / 32768.0


def measure(a, ref):
    """The project's feature measure |a - ref| / max(1, |ref|) (bound 1e-4), element-wise, in float64."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(a - ref) / np.maximum(1.0, np.abs(ref))


def _one_thread(fn):
    """The references are thousands of small tensor operations, several times faster without torch's thread pool than with
    it; the caller's thread count is put back."""
    @functools.wraps(fn)
    def wrapped(*args):
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            return fn(*args)
        finally:
            torch.set_num_threads(n)
    return wrapped


def _fwd_one(x):
    r64 = features_ref.extract_features_f64(x.numpy(), stages=True, max_duration=LONG)
    r32 = features_ref.extract_features_f32(x, max_duration=LONG, stages=True)
    return r64, r32


@functools.lru_cache(maxsize=None)
@_one_thread
def fwd_reference(kind):
    """kind "f32" / "i16" -> dict over the forward sweep (N = len(fwd_cases())):
    wave   float32 [N, Lmax] (zero behind each clip; for "i16" the dequantised values), pcm int16 [N, Lmax] ("i16" only)
    db64, norm64   float64 [N, 64, T_PAD], zero behind each clip's T frames
    frames int [N];  mel_min float: the smallest float64 mel power of the sweep
    o32_db, o32_norm  float [N]: the float32 oracle's worst ``measure`` against float64, per clip."""
    cases = fwd_cases()
    lmax = max(n for _, n in cases)
    wave = torch.zeros(len(cases), lmax)
    db64 = np.zeros((len(cases), 64, T_PAD))
    norm64 = np.zeros((len(cases), 64, T_PAD))
    o32_db, o32_norm = np.zeros(len(cases)), np.zeros(len(cases))
    mel_min = np.inf
    for i, (t, n) in enumerate(cases):
        x = clip(t, n)
        if kind == "i16":
            x = dequantise(quantise(x))
        wave[i, :n] = x
        r64, r32 = _fwd_one(x)
        assert r64["db"].shape == (64, t) and tuple(r32["db"].shape) == (64, t)
        db64[i, :, :t], norm64[i, :, :t] = r64["db"], r64["norm"]
        o32_db[i] = measure(r32["db"].numpy(), r64["db"]).max()
        o32_norm[i] = measure(r32["norm"].numpy(), r64["norm"]).max()
        mel_min = min(mel_min, r64["mel_power"].min())
    ref = {"wave": wave, "db64": db64, "norm64": norm64, "frames": np.array([t for t, _ in cases]),
           "o32_db": o32_db, "o32_norm": o32_norm, "mel_min": float(mel_min)}
    if kind == "i16":
        ref["pcm"] = (wave * 32768.0).to(torch.int16)              # exact: every value is q / 32768
    return ref


def dout_batch(n, seed):
    return torch.randn(n, 64, T_PAD, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
@_one_thread
def bwd_reference(kind):
    """kind "f32" / "i16" -> dict over the backward sweep: wave [N, Lmax] (dequantised for "i16", with pcm beside it), dout
    [N, 64, T_PAD], g64 (list of float64 [L]), e32 float [N]: ``clip_error`` of the float32 autograd gradient against g64."""
    cases = bwd_cases()
    lmax = max(n for _, n in cases)
    wave = torch.zeros(len(cases), lmax)
    dout = dout_batch(len(cases), seed=7)
    g64, e32 = [], np.zeros(len(cases))
    for i, (t, n) in enumerate(cases):
        x = clip(t, n)
        if kind == "i16":
            x = dequantise(quantise(x))
        wave[i, :n] = x
        g = gref.grad_f64(x, dout[i])
        g64.append(g)
        e32[i] = gref.clip_error(gref.grad_f32(x, dout[i]), g)
    ref = {"wave": wave, "dout": dout, "g64": g64, "e32": e32}
    if kind == "i16":
        ref["pcm"] = (wave * 32768.0).to(torch.int16)
    return ref


def fold_sample(t):
    """The sample the last padded position of a clip of 512 (T - 1) samples reflects onto."""
    return HOP * (t - 2) - 1


def fold_cases():
    """The backward lengths that are a multiple of the hop: the last padded sample, 512 T - 1, reflects onto 512 (T - 2) - 1."""
    return [(t, n) for t, n in bwd_cases() if n == HOP * (t - 1)]


@functools.lru_cache(maxsize=None)
@_one_thread
def fold_reference(kind):
    """The clips of ``fold_cases()`` with a ``dout`` that is zero but on the last frame.  The last padded sample carries the
    Hann weight w[1023] = 9.4e-6, so under a full ``dout`` what it folds back is below the float32 rounding of the sample it lands
    on (measured: median 7e-7, at most 1.7e-5 of the clip's rms); with the last frame alone feeding the gradient, frame T - 2
    -- whose centre that sample is -- carries only the z-norm's coupling terms and the fold stands clear of its rounding.
    -> wave [M, Lmax], pcm ("i16"), dout [M, 64, T_PAD], g64 (list), fold [M]: d loss / d (last padded sample) in float64, the part
    of g64[512 (T - 2) - 1] that comes from there."""
    cases = fold_cases()
    lmax = max(n for _, n in cases)
    wave = torch.zeros(len(cases), lmax)
    dout = torch.zeros(len(cases), 64, T_PAD)
    full = dout_batch(len(cases), seed=9)
    g64, fold = [], np.zeros(len(cases))
    for i, (t, n) in enumerate(cases):
        x = clip(t, n)
        if kind == "i16":
            x = dequantise(quantise(x))
        wave[i, :n] = x
        dout[i, :, t - 1] = full[i, :, t - 1]
        g = gref.grad_f64(x, dout[i])
        g64.append(g)
        xp = torch.nn.functional.pad(x.double()[None, None], (HOP, HOP), mode="reflect")[0, 0].requires_grad_(True)
        out = gref.features_from_padded_f64(xp, t_pad=T_PAD)
        (gp,) = torch.autograd.grad((out * dout[i].double()).sum(), xp)
        fold[i] = gp[-1].item()
        # (the padded gradient folded by hand is the gradient: sample 512 (T - 2) - 1 holds its own position's and the last one's
        # -- and at T = 3, where it is sample 511, the head's position -511 as well)
        k = fold_sample(t)
        by_hand = gp[HOP + k].item() + fold[i] + (gp[HOP - k].item() if k <= HOP else 0.0)
        assert abs(by_hand - g[k].item()) <= 1e-9 * g.abs().max().item(), (t, n)
    ref = {"wave": wave, "dout": dout, "g64": g64, "fold": fold}
    if kind == "i16":
        ref["pcm"] = (wave * 32768.0).to(torch.int16)
    return ref


def aug_time_mask(t):
    return (t - 1, 5)                             # from the last frame across the clip's end


@functools.lru_cache(maxsize=None)
@_one_thread
def aug_reference():
    """Dict over ``aug_cases()``: wave [N, Lmax], dout [N, 64, T_PAD] with 1e6 / -1e6 at the masked positions (a leak is not
    small), out64 float64 [N, 64, T_PAD], g64 (list), e32 [N], constant [N] (bool: the augmented clip has a constant dB tile, its
    features and its gradient are exact zeros), dead [N] (bool: every sample is shifted out of the clip, so the features are those
    of the noise and the gradient is exact zeros: nothing to take a ratio against), db_min: the smallest float64 dB value before
    normalisation."""
    cases = aug_cases()
    lmax = max(n for _, n, _ in cases)
    wave = torch.zeros(len(cases), lmax)
    dout = dout_batch(len(cases), seed=8)
    out64 = np.zeros((len(cases), 64, T_PAD))
    g64, e32, constant, dead = [], np.zeros(len(cases)), np.zeros(len(cases), dtype=bool), np.zeros(len(cases), dtype=bool)
    db_min = np.inf
    for i, (t, n, s) in enumerate(cases):
        x = clip(t, n)
        wave[i, :n] = x
        tm = aug_time_mask(t)
        dout[i, :, tm[0]: tm[0] + tm[1]] = 1e6
        dout[i, AUG_FREQ_MASK[0]:, :] = -1e6
        noise = torch.from_numpy(host_rng.gauss_noise(AUG_SEED, i, n)).double() * AUG_SIGMA
        kw = dict(shift=s, noise=noise, time_mask=tm, freq_mask=AUG_FREQ_MASK)
        out64[i] = gref.features_f64(x.double(), t_pad=T_PAD, **kw).numpy()
        xa = (gref.shifted(x.double(), s) + noise).numpy()
        db = features_ref.extract_features_f64(xa, stages=True, max_duration=LONG)["db"]
        db_min = min(db_min, db.min())
        constant[i] = db.std() == 0.0
        g = gref.grad_f64(x, dout[i], **kw)
        g64.append(g)
        dead[i] = abs(s) >= n
        assert dead[i] == bool((g == 0).all()) or constant[i]
        e32[i] = 0.0 if constant[i] or dead[i] else gref.clip_error(gref.grad_f32(x, dout[i], **kw), g)
    return {"wave": wave, "dout": dout, "out64": out64, "g64": g64, "e32": e32, "constant": constant, "dead": dead,
            "db_min": float(db_min)}


def gen_empty_filters(cfg):
    """Filters of the handle's bank that cover no FFT bin (n_fft 256 has one): exactly -100 dB on both sides, by construction."""
    fb = cref.htk_mel_fbanks(cfg[0] // 2 + 1, 0.0, float(cref.SAMPLE_RATE // 2), cref.N_MELS, cref.SAMPLE_RATE)
    return [j for j in range(cref.N_MELS) if not (fb[:, j] != 0).any()]


@functools.lru_cache(maxsize=None)
@_one_thread
def gen_reference(cfg):
    """cfg (n_fft, hop, win) -> dict over ``gen_cases(cfg)``: waves (list of float32 [L]), db64 / norm64 float64 [N, 64,
    GEN_T_PAD], frames [N], o32_db / o32_norm [N] as in ``fwd_reference``."""
    n_fft, hop, win = cfg
    cases = gen_cases(cfg)
    waves = []
    db64 = np.zeros((len(cases), 64, GEN_T_PAD))
    norm64 = np.zeros((len(cases), 64, GEN_T_PAD))
    o32_db, o32_norm = np.zeros(len(cases)), np.zeros(len(cases))
    for i, (t, n) in enumerate(cases):
        x = cref.chirp_clips(1, n, seed=100 + t)[0]
        waves.append(x)
        r64 = cref.features_f64(x.numpy(), n_fft, hop, win)
        r32 = cref.features_f32(x, n_fft, hop, win)
        assert r64["db"].shape == (64, t)
        db64[i, :, :t], norm64[i, :, :t] = r64["db"], r64["norm"]
        o32_db[i] = measure(r32["db"].numpy(), r64["db"]).max()
        o32_norm[i] = measure(r32["norm"].numpy(), r64["norm"]).max()
    return {"waves": waves, "db64": db64, "norm64": norm64, "frames": np.array([t for t, _ in cases]),
            "o32_db": o32_db, "o32_norm": o32_norm}
