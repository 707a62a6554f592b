"""float64 oracle of sir_wave_reverb_mix, written from its definition (include/sir_hip.h), one row at a time.

reverb  y[n] = sum_{k < min(K, n + 1)} x[n - k] h[k], n in [0, L): ``np.convolve`` cut at L
noise   out[n] = y[n] + g v[(o + n) mod M],  g = sqrt(P_y / (P_v 10^(snr_db / 10))),  P_y = mean y^2 over [0, L),  P_v = mean
        square of the L noise samples used;  g = 0 when P_y or P_v is 0;  a g that is no finite float32 (an extreme snr_db)
        makes the row a bad one: zeroed, gain 0

``ols_ring_model`` is no second oracle: it restates the kernel's schedule (partitions, rounds, the spectrum ring) in float32 so
that a CPU test can show which cases tell a correct ring from a broken one.
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
    """-> (g, whether float32(g) is finite).  Total over finite snr_db: 10^(snr / 10) overflowing to inf gives g = 0, underflowing
    to 0 gives g = inf."""
    if len(y) == 0:
        return 0.0, True
    p_y, p_v = float(np.mean(y * y)), float(np.mean(used * used))
    if p_y == 0.0 or p_v == 0.0:
        return 0.0, True
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        ratio = np.power(np.float64(10.0), np.float64(snr_db) / 10.0)
        g = np.sqrt(np.float64(p_y) / (np.float64(p_v) * ratio))
        return float(g), bool(np.isfinite(np.float32(g)))


def mix_row(x, h=None, v=None, offset=0, snr_db=0.0):
    """-> (out [L], y [L], g, used [L] or None), all float64; a gain that is no finite float32: out = 0, g = 0"""
    y = reverb(x, h)
    if v is None:
        return y.copy(), y, 0.0, None
    used = wrapped(v, offset, len(y))
    g, finite = noise_gain(y, used, snr_db)
    if not finite:
        return np.zeros_like(y), y, 0.0, used
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


def ols_ring_model(x, h, parts, ring_extra=3, waves=4, part=512):
    """The kernel's overlap-save schedule in numpy float32 / complex64.  x [L], h [K] with ceil(K / 512) <= parts -> y [L] float32.

    H_p = rfft of taps [512 p, 512 p + 512) zero-padded to 1024, times 1 / 1024.  Blocks go in rounds of ``waves``: every block m
    of a round first stores the spectrum X_m of the window [512 (m - 1), 512 (m + 1)) in ring[m % R], R = parts + ring_extra;
    then every block of the round sums H_p ring[(m - p) mod R] over p < min(P, m + 1), the index walking down from m % R with
    wrap, and takes the second half of the inverse transform (times 1024) as samples [512 m, 512 m + 512)."""
    x, h = np.asarray(x, dtype=np.float32), np.asarray(h, dtype=np.float32)
    n, k = len(x), len(h)
    n_part = -(-k // part)
    assert x.ndim == h.ndim == 1 and k >= 1 and n_part <= parts
    size = 2 * part
    taps = np.zeros((n_part, size), dtype=np.float32)
    for p in range(n_part):
        seg = h[part * p:part * (p + 1)]
        taps[p, :len(seg)] = seg
    hs = (np.fft.rfft(taps, axis=1) * np.float32(1.0 / size)).astype(np.complex64)
    r = parts + ring_extra
    ring = np.zeros((r, part + 1), dtype=np.complex64)
    padded = np.zeros(part + (-(-n // part) + 1) * part, dtype=np.float32)      # x behind `part` zeros: window m starts at 512 m
    padded[part:part + n] = x
    y = np.zeros(n, dtype=np.float32)
    n_blk = -(-n // part)
    for m0 in range(0, n_blk, waves):
        blocks = range(m0, min(m0 + waves, n_blk))
        for m in blocks:
            ring[m % r] = np.fft.rfft(padded[part * m:part * m + size]).astype(np.complex64)
        for m in blocks:
            acc = np.zeros(part + 1, dtype=np.complex64)
            s = m % r
            for p in range(min(n_part, m + 1)):
                acc += hs[p] * ring[s]
                s = r - 1 if s == 0 else s - 1
            blk = (np.fft.irfft(acc, size) * np.float32(size)).astype(np.float32)[part:]
            y[part * m:part * (m + 1)] = blk[:n - part * m]
    return y
