"""Cases shared by tests/test_perturb_geometry_gpu.py and tests/test_perturb_geometry_host.py: the WSOLA geometry
(S, W, O, H) at every sample rate the perturbation tests visit, the row lengths placed around it, the clips, and a float32
emulation of the search (what a float32 kernel may legitimately pick against the float64 contract of wave_perturb_ref)."""
import numpy as np
import torch

import wave_perturb_ref as ref
from sir_amd import synth

# sr -> (S, W, O, H), sox tempo.c's formulas (ref.geometry / geom_for in csrc/perturb.hip)
GEOMETRY = {
    8000: (656, 117, 96, 560),          # W < 128: waves 2 and 3 of the argmin carry only the sentinel
    8500: (697, 125, 104, 593),         # H odd: no 16-byte stores anywhere, unaligned segment bases
    11025: (904, 162, 136, 768),
    16000: (1312, 235, 192, 1120),
    22050: (1808, 324, 264, 1544),      # W > 256: a thread owns two candidates
    24000: (1968, 352, 288, 1680),      # W + S = 2320 of 2368, O = 288 = the kernel's limit
}
RATES = [8000, 8500, 11025, 22050, 24000]                 # 16 000 is tests/test_wave_perturb_gpu.py's
TEMPO_FACTORS = [0.5, 0.7, 0.85, 1.15, 1.5, 2.0]
PITCH_CENTS = [-200.0, -37.5, 150.0, 200.0]


def lengths_for(sr):
    S, W, O, H = ref.geometry(sr)
    return [2 * sr, 0, 1, W // 2, H - 1, H, H + 1, S, 2 * H, 3 * H + 7, 2 * sr - 1]


def max_segments(sr):
    """Segments of the longest output (max_len at tempo 0.5), plus one."""
    H = ref.geometry(sr)[3]
    return -(-2 * (2 * sr) // H) + 1


def round_up4(n):
    return (int(n) + 3) // 4 * 4


def clips(sr, dtype=torch.float32, seed=77):
    """[11, 2 sr] clips of lengths_for(sr), zero beyond their length."""
    lens = lengths_for(sr)
    x = synth.synth_clips(len(lens), 2 * sr, seed=seed + sr)
    if dtype == torch.int16:
        x = (x * 32767.0).round().to(torch.int16)
    for b, n in enumerate(lens):
        x[b, n:] = 0
    return x


def host_f64(x, b, n):
    return x[b, :n].double().numpy() / (32768.0 if x.dtype == torch.int16 else 1.0)


def per_row_factors(n, seed=3):
    """One float32 draw per row from [0.5, 2]."""
    return np.random.default_rng(seed).uniform(0.5, 2.0, n).astype(np.float32)


def tempo_offsets_f32(x, f, sr):
    """The offsets a float32 search picks: z and the tail `ob` held in float32, the cross-fade in float32, each cost
    accumulated term by term in float32, first minimum."""
    x = np.asarray(x, dtype=np.float32)
    f = float(f)
    S, W, O, H = ref.geometry(sr)
    L = len(x)
    N = ref.out_len(L, f)
    nseg = -(-N // H)
    hw = W // 2
    p_last = int(f * (nseg - 1) * H + 0.5) if nseg > 1 else 0
    z = np.zeros(max(p_last + W + S, hw + L) + 1, dtype=np.float32)
    z[hw:hw + L] = x
    ob, used = None, []
    for j in range(nseg):
        p = 0 if j == 0 else int(f * j * H + 0.5)
        if j == 0:
            off = hw
        else:
            acc = np.zeros(W, dtype=np.float32)
            for m in range(O):
                d = z[p + m:p + m + W] - ob[m]
                acc = acc + d * d
            off = int(np.argmin(acc))
        used.append(off)
        ob = z[p + off + H:p + off + S].copy()
    return used


def tie_clip(sr, first_zero_candidate, n=None):
    """A clip of ``n`` samples (default 2 sr) that is a burst followed by exact zeros, cut so that at tempo 0.5 segment 1
    has the all-zero tail ob and candidates [first_zero_candidate, W) whose windows are all zero: they tie at cost 0
    exactly, in any precision, and every lower candidate costs more.  The first minimum is first_zero_candidate; every
    later segment ties over all of [0, W) and picks 0."""
    S, W, O, H = ref.geometry(sr)
    n = 2 * sr if n is None else n
    p1 = int(0.5 * H + 0.5)
    k = p1 - W // 2 + first_zero_candidate          # candidate i reads x[p1 - W/2 + i ...]: zero from i = first_zero_candidate on
    assert 0 < k <= H and 0 <= first_zero_candidate < W
    x = synth.synth_clips(1, n, seed=1000 + first_zero_candidate)[0]
    x[k - 1] = 0.25                                 # the last sample of the burst is not a chance zero
    x[k:] = 0
    return x
