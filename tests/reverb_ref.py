"""float64 oracle of sir_wave_reverb_mix, written from its definition (include/sir_hip.h), one row at a time.

reverb  y[n] = sum_{k < min(K, n + 1)} x[n - k] h[k], n in [0, L): ``np.convolve`` cut at L
noise   out[n] = y[n] + g v[(o + n) mod M],  g = sqrt(P_y / (P_v 10^(snr_db / 10))),  P_y = mean y^2 over [0, L),  P_v = mean
        square of the L noise samples used;  g = 0 when P_y or P_v is 0
"""
import numpy as np


def reverb(x, h):
    """x [L], h [K] (K >= 1) -> y [L] float64; h None = no reverb."""
    x = np.asarray(x, dtype=np.float64)
    if h is None or len(x) == 0:
        return x.copy()
    h = np.asarray(h, dtype=np.float64)
    assert h.ndim == 1 and len(h) >= 1
    return np.convolve(x, h)[:len(x)]


def wrapped(v, offset, n):
    """the n noise samples used: v[(offset + i) mod M], i in [0, n)"""
    v = np.asarray(v, dtype=np.float64)
    assert v.ndim == 1 and len(v) >= 1
    return v[(int(offset) + np.arange(n, dtype=np.int64)) % len(v)]


def noise_gain(y, used, snr_db):
    if len(y) == 0:
        return 0.0
    p_y, p_v = float(np.mean(y * y)), float(np.mean(used * used))
    if p_y == 0.0 or p_v == 0.0:
        return 0.0
    return float(np.sqrt(p_y / (p_v * 10.0 ** (float(snr_db) / 10.0))))


def mix_row(x, h=None, v=None, offset=0, snr_db=0.0):
    """-> (out [L], y [L], g, used [L] or None), all float64"""
    y = reverb(x, h)
    if v is None:
        return y.copy(), y, 0.0, None
    used = wrapped(v, offset, len(y))
    g = noise_gain(y, used, snr_db)
    return y + g * used, y, g, used


def mix_batch(wave, lengths, rirs=None, rir_index=None, noises=None, noise_index=None, noise_offset=None, snr_db=None):
    """wave [B, >= max L] (float; PCM16 already dequantised), rirs / noises: lists of 1-D arrays.  -> list of mix_row results"""
    res = []
    for b, n in enumerate(lengths):
        r = -1 if rir_index is None else int(rir_index[b])
        q = -1 if noise_index is None else int(noise_index[b])
        res.append(mix_row(np.asarray(wave[b][:n], dtype=np.float64), rirs[r] if r >= 0 else None, noises[q] if q >= 0 else None,
                           0 if q < 0 else int(noise_offset[b]), 0.0 if q < 0 else float(snr_db[b])))
    return res
