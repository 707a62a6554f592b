"""Float64 statement of the pitch / tempo perturbation contract (``sir_wave_perturb``).

Tempo ``T(x, f)`` restates sox 14.4's ``tempo`` effect (default profile, linear search) at the handle's sample rate;
pitch ``P(x, c)`` is ``T(x, 1/d)``, d = 2^(c/1200), resampled back to ``len(x)`` samples at the fractional positions
``n d`` with the library's windowed-sinc filter (sinc_interp_hann, width 6, rolloff 0.99).  sox is not available to the
tests, so no sample-level parity with it is claimed: THIS is the contract.

WSOLA's argmin is discontinuous: a float32 evaluation may pick another offset than float64 at a near-tie.  Both
functions therefore accept the offsets a kernel chose (``offsets``) and then rebuild the output from them, still
returning, per segment j >= 1, the float64 costs of every candidate under the tail that those offsets produced.
"""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def geometry(sr=16000):
    """(S, W, O, H): segment, search, overlap and hop in samples (sox tempo.c's formulas; 1312, 235, 192, 1120 at 16 kHz)."""
    S = int(sr * 82 / 1000 + .5)
    W = int(sr * 14.68 / 1000 + .5)
    O = int(max(sr * 12 / 1000 + 4.5, 16)) & ~7
    if 2 * O > S:
        O -= 8
    return S, W, O, S - O


def out_len(length, f):
    """int(L / f + 0.5) in double; 1.0 is the identity."""
    f = float(f)
    return int(length) if f == 1.0 else int(int(length) / f + 0.5)


def tempo(x, f, sr=16000, offsets=None):
    """-> (y [int(L/f + .5)] float64, offsets used [n_segments], costs [one float64 [W] array per segment j >= 1])."""
    x = np.asarray(x, dtype=np.float64)
    f = float(f)
    if f == 1.0:
        return x.copy(), [], []
    S, W, O, H = geometry(sr)
    L = len(x)
    N = out_len(L, f)
    nseg = -(-N // H)
    hw = W // 2
    p_last = int(f * (nseg - 1) * H + 0.5) if nseg > 1 else 0
    z = np.zeros(max(p_last + W + S, hw + L) + 1)
    z[hw:hw + L] = x
    out = np.zeros(nseg * H)
    ramp = np.arange(O) / O
    ob, used, costs = None, [], []
    for j in range(nseg):
        p = 0 if j == 0 else int(f * j * H + 0.5)
        if j == 0:
            off = hw
        else:
            c = ((sliding_window_view(z[p:p + W + O - 1], O) - ob) ** 2).sum(axis=1)
            costs.append(c)
            off = int(np.argmin(c)) if offsets is None else int(offsets[j])
        used.append(off)
        q = p + off
        seg = z[q:q + H].copy()
        if j > 0:
            seg[:O] = ob * (1.0 - ramp) + z[q:q + O] * ramp
        out[j * H:(j + 1) * H] = seg
        ob = z[q + H:q + S].copy()
    return out[:N], used, costs


def resample_frac(s, d, length):
    """y[n] = sum_k s[k] h(n d - k), n < length; h(u) = b sinc(t) cos(pi t / 12)^2, t = clip(u b, -6, 6),
    b = 0.99 min(1, 1/d); s is zero outside its length."""
    s = np.asarray(s, dtype=np.float64)
    b = 0.99 * min(1.0, 1.0 / d)
    R = 6.0 / b
    pos = np.arange(int(length), dtype=np.float64) * d
    K = int(math.ceil(2 * R)) + 3
    k = np.floor(pos - R)[:, None].astype(np.int64) + np.arange(K)[None, :]
    t = np.clip((pos[:, None] - k) * b, -6.0, 6.0)
    h = b * np.sinc(t) * np.cos(np.pi * t / 12.0) ** 2
    inside = (k >= 0) & (k < len(s))
    sv = np.where(inside, s[np.clip(k, 0, max(len(s) - 1, 0))] if len(s) else 0.0, 0.0)
    return (sv * h).sum(axis=1)


def pitch(x, cents, sr=16000, offsets=None):
    """-> (y [L] float64, offsets used, costs, stretched signal s = T(x, 1/d))."""
    x = np.asarray(x, dtype=np.float64)
    c = float(cents)
    if c == 0.0:
        return x.copy(), [], [], x.copy()
    d = 2.0 ** (c / 1200.0)
    s, used, costs = tempo(x, 1.0 / d, sr, offsets)
    return resample_frac(s, d, len(x)), used, costs, s


def shifted(x, shift):
    """x_s[i] = x[i - shift] inside [0, L), zero elsewhere (sir_augment.shift)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    L, s = len(x), int(shift)
    if s >= 0:
        out[s:] = x[:max(L - s, 0)]
    else:
        out[:max(L + s, 0)] = x[-s:]
    return out
