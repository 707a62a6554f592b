"""float64 references and case lists of the waveform front end (csrc/frontend.hip: ``sir_resample``, ``sir_mix_to_mono``) for
tests/test_frontend_edge_host.py and tests/test_frontend_edge_gpu.py.  Numpy only: no torch, no device.

The resampler is torchaudio's ``sinc_interp_hann`` (lowpass_filter_width 6, rolloff 0.99).  With the rates reduced by their gcd
to ``orig`` and ``nw``, ``base = 0.99 min(orig, nw)``, ``scale = base / orig`` and output sample ``j = n nw + p``:

    phi_p     = float64(float32(-p) / float32(nw))          torchaudio's float32 phase term, part of the definition
    tt        = (phi_p + (i - n orig) / orig) base
    h64(j, i) = scale sinc(pi tt) cos^2(pi tt / 12)          if |tt| < 6, else 0
    y[j]      = sum_i x[i] h64(j, i),   S[j] = sum_i |x[i]| |h64(j, i)|,   0 <= i < len,   j < ceil(nw len / orig)

``h64`` evaluates that one (j, i) pair at a time (vectorised); nothing here keeps a polyphase table, a first-tap index or a
convolution.  ``resample64`` sums over the input offsets ``i - n orig`` in ``[-width - 2, width + orig + 2]``: every offset
outside that range has |tt| >= 6 (``width = ceil(6 orig / base)``, phi in (-1, 0]), and the window test stays ``h64``'s own, so
the range only saves work (``resample64_dense`` sums over every i; the host tests compare the two).

Bounds (u = 2^-24), derived from the kernel's arithmetic -- one fmaf chain over float32 taps, a zero tap or a zero sample
leaves the accumulator as it is:
  random signal   |dev - y| <= (m(p) + 1) u S[j],  m(p) = nonzero taps of phase p: one u for each tap's own rounding, m for the chain
  single impulse  |dev - y| <= 2^-23 |y| + 2^-149  (one product, nothing accumulated: the float32 tap itself), exactly 0 where y is 0
  mono, int16     dev == float32(sum_c s_c / (32768 channels)) bit for bit: every s / 32768 is a multiple of 2^-15 and 64 of them
                  need 21 bits, so the float32 sum is exact and the one division is correctly rounded.  (The float64 quotient
                  formed here rounds to the same float32: it is at least 2^-31 relative away from any float32 midpoint it does
                  not hit, far more than its own 2^-53.)
  mono, float32   |dev - mean64| <= u sum_c |x_c| (1 + 64 u): (c - 1) roundings of the sum, divided by c, plus the quotient's own
"""
import math

import numpy as np

U = 2.0 ** -24
LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99

PAIRS = [(44100, 8000), (48000, 8000), (16000, 8000), (22050, 8000), (11025, 16000), (12000, 16000), (32000, 16000),
         (96000, 16000), (22050, 16000), (44100, 16000), (16000, 22050), (16000, 48000), (16000, 44100), (8000, 48000),
         (44100, 48000), (48000, 44100)]
RANDOM_PAIRS = [(44100, 8000), (11025, 16000), (16000, 44100), (48000, 8000), (12000, 16000), (22050, 16000)]
BLOCK_TARGETS = (255, 256, 257, 511, 512, 513)          # output lengths around the edges of the kernel's 256-thread blocks
MONO_CHANNELS = [1, 2, 3, 5, 6, 7, 8, 63, 64]


def reduced(orig_freq, new_freq):
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // g, int(new_freq) // g


def width(orig_freq, new_freq):
    orig, nw = reduced(orig_freq, new_freq)
    return math.ceil(LOWPASS_FILTER_WIDTH * orig / (min(orig, nw) * ROLLOFF))


def out_len(length, orig_freq, new_freq):
    """ceil(nw length / orig) in Python integers."""
    orig, nw = reduced(orig_freq, new_freq)
    return -((-nw * int(length)) // orig)


def h64(orig_freq, new_freq, j, i):
    """The filter's weight of input sample i in output sample j, float64 (j, i: integer arrays, broadcast)."""
    orig, nw = reduced(orig_freq, new_freq)
    base = min(orig, nw) * ROLLOFF
    scale = base / orig
    j, i = np.asarray(j, dtype=np.int64), np.asarray(i, dtype=np.int64)
    n, p = j // nw, j % nw
    phi = ((-p).astype(np.float32) / np.float32(nw)).astype(np.float64)
    tt = (phi + (i - n * orig) / orig) * base
    inside = np.abs(tt) < LOWPASS_FILTER_WIDTH
    window = np.cos(tt * math.pi / LOWPASS_FILTER_WIDTH / 2) ** 2
    a = tt * math.pi
    sinc = np.where(a == 0, 1.0, np.sin(a) / np.where(a == 0, 1.0, a))
    return np.where(inside, sinc * (window * scale), 0.0)


def offsets(orig_freq, new_freq):
    """Input offsets i - n orig that can lie inside the window, with a margin of two on each side."""
    orig, _ = reduced(orig_freq, new_freq)
    w = width(orig_freq, new_freq)
    return np.arange(-(w + 2), w + orig + 3, dtype=np.int64)


def taps64(orig_freq, new_freq):
    """-> (d, H): H[p, k] = h64 of phase p at input offset d[k] (n = 0), over ``offsets``."""
    _, nw = reduced(orig_freq, new_freq)
    d = offsets(orig_freq, new_freq)
    return d, h64(orig_freq, new_freq, np.arange(nw)[:, None], d[None, :])


def nonzero_taps(orig_freq, new_freq):
    """m(p): how many taps of phase p are not zero."""
    return (taps64(orig_freq, new_freq)[1] != 0).sum(axis=1)


def resample64(x, orig_freq, new_freq):
    """-> (y, S) float64 of the first docstring, for one clip x (1-D)."""
    orig, nw = reduced(orig_freq, new_freq)
    x = np.asarray(x, dtype=np.float64)
    t = out_len(len(x), orig_freq, new_freq)
    if t == 0:
        return np.zeros(0), np.zeros(0)
    j = np.arange(t, dtype=np.int64)
    i = (j // nw)[:, None] * orig + offsets(orig_freq, new_freq)[None, :]
    valid = (i >= 0) & (i < len(x))
    xi = np.where(valid, x[np.clip(i, 0, len(x) - 1)], 0.0)
    h = np.where(valid, h64(orig_freq, new_freq, j[:, None], i), 0.0)
    return (xi * h).sum(axis=1), (np.abs(xi) * np.abs(h)).sum(axis=1)


def resample64_dense(x, orig_freq, new_freq):
    """``resample64`` with the sums over every input sample (small clips only)."""
    x = np.asarray(x, dtype=np.float64)
    t = out_len(len(x), orig_freq, new_freq)
    h = h64(orig_freq, new_freq, np.arange(t)[:, None], np.arange(len(x))[None, :])
    return (x[None, :] * h).sum(axis=1), (np.abs(x)[None, :] * np.abs(h)).sum(axis=1)


def resample_bound(S, orig_freq, new_freq):
    """(m(p) + 1) u S[j] for the outputs j = 0 .. len(S) - 1."""
    _, nw = reduced(orig_freq, new_freq)
    m = nonzero_taps(orig_freq, new_freq)
    return (m[np.arange(len(S)) % nw] + 1) * U * S


# ---- impulses: every tap of every phase -------------------------------------------------------------------------------------
def impulse_case(orig_freq, new_freq):
    """-> (length, positions): one row per residue r in [0, orig) with its impulse at ``positions[r]`` = r + k0 orig, far enough
    from both ends that every output the impulse reaches exists (tap (p, d) is met by the row r = d mod orig at n =
    (q - d) / orig: n >= 0 because q >= width + 2 + orig >= d, and j < (q + width + 2 + orig) nw / orig <= the output length);
    then two more rows, the impulse at sample 0 and at sample length - 1."""
    orig, _ = reduced(orig_freq, new_freq)
    w = width(orig_freq, new_freq)
    k0 = -(-(w + 2) // orig) + 1
    q = [r + k0 * orig for r in range(orig)]
    length = q[-1] + w + orig + 3
    return length, q + [0, length - 1]


def impulse64(q, amplitude, length, orig_freq, new_freq):
    """y of a clip of ``length`` samples that is ``amplitude`` at sample q and zero elsewhere: amplitude h64(j, q)."""
    return amplitude * h64(orig_freq, new_freq, np.arange(out_len(length, orig_freq, new_freq)), q)


def impulse_bound(y):
    return 2.0 ** -23 * np.abs(y) + 2.0 ** -149


# ---- random signals at the length edges -------------------------------------------------------------------------------------
def edge_lengths(orig_freq, new_freq):
    """0..3, the filter's half support and one more, one input period less / exactly / more, two periods and one, and for each
    output length of BLOCK_TARGETS the smallest clip that has it (when up-converting, output lengths skip values: then the
    smallest clip whose output reaches it)."""
    orig, nw = reduced(orig_freq, new_freq)
    w = width(orig_freq, new_freq)
    out = [0, 1, 2, 3, w, w + 1, orig - 1, orig, orig + 1, 2 * orig + 1]
    for target in BLOCK_TARGETS:
        length = ((target - 1) * orig) // nw + 1
        assert out_len(length, orig_freq, new_freq) >= target > out_len(length - 1, orig_freq, new_freq)
        out.append(length)
    return list(dict.fromkeys(out))


def random_case(orig_freq, new_freq):
    """-> dict: ``lengths`` as passed to the kernel (int32), ``used`` the lengths it must act on, ``f32`` [B, max_len] float32 with
    NaN at and behind each row's length, ``i16`` the same clips as int16 with 32767 there.  The last two rows: a full row whose
    length says max_len + 1000 (read as max_len) and a row of poison whose length says -1000 (an empty clip)."""
    lens = edge_lengths(orig_freq, new_freq)
    max_len = max(lens) + 7
    rng = np.random.Generator(np.random.PCG64(orig_freq * 100003 + new_freq))
    used = lens + [max_len, 0]
    given = lens + [max_len + 1000, -1000]
    f32 = np.full((len(used), max_len), np.nan, dtype=np.float32)
    i16 = np.full((len(used), max_len), 32767, dtype=np.int16)
    for b, n in enumerate(used):
        x = (0.3 * rng.standard_normal(n)).astype(np.float32)
        f32[b, :n] = x
        i16[b, :n] = np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)
    return {"lengths": np.asarray(given, dtype=np.int32), "used": used, "f32": f32, "i16": i16}


# ---- mono ---------------------------------------------------------------------------------------------------------------------
def mono_i16_exact(pcm):
    """pcm int16 [frames, channels] -> float32 [frames], the correctly rounded mean of s / 32768 (module docstring)."""
    pcm = np.asarray(pcm)
    return (pcm.astype(np.int64).sum(axis=1).astype(np.float64) / (32768.0 * pcm.shape[1])).astype(np.float32)


def mono_f32(pcm):
    """pcm float32 [frames, channels] -> (mean64, bound)."""
    x = np.asarray(pcm, dtype=np.float64)
    return x.mean(axis=1), U * np.abs(x).sum(axis=1) * (1.0 + 64.0 * U)
