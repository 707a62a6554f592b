"""The case table that holds sir_wave_reverb_mix's spectrum ring to the float64 oracle at every ring size, shared by
test_reverb_scale_host.py (which shows on the CPU that each case tells a correct ring from a broken one) and
test_reverb_scale_gpu.py (which runs the kernel on them).

One call per max_rir_len: 512 p for p = 1 .. 16, then 1, 513 and 8191.  parts = ceil(max_rir_len / 512) sizes the kernel's LDS,
R = parts + 3 is its ring, and max_len = 512 (2 R + 5) is two ring revolutions and part of a third.  The rows of a call:

  row  RIR                                               length
  0    flat, K = max_rir_len                             max_len
  1    lone, K = 512 (parts - 1) + 1, last tap +-0.5     max_len - 7
  2    decay, K = max_rir_len, last tap -+0.5            max_len - 511
  3    one, K = 1                                        max_len - 512                 (one block fewer)
  4    flat again (two rows share a RIR)                 512 (blocks - 2) - 100        (two fewer)
  5    lone again                                        512 (blocks - 3) - 37         (three fewer)
  6    index -1                                          max_len - 1000
  7    short, K = 512 (parts - 1) (P < parts), where >= 1  max_len of the call with max_rir_len = K, on waveform 0

blocks = 2 R + 5 is odd, so the four block counts end in rounds of 1, 2, 3 and 4 blocks.  A flat RIR is 0.2 N(0, 1) with h[0] = 1,
the first K taps of ONE sequence: every partition carries an equal share of |h|_1, and row 7 of a call is row 0 of the call one
partition smaller (same taps, waveform and length), which is how the GPU test shows that the ring's size does not change a row's
bits.  The lone tap of a last partition is +-0.5 because a random one of 0.2 N(0, 1) can be too small to show when it is lost; the
60 dB decay (synth.synthetic_rir) ends in a late echo of the same size for the same reason.
"""
import functools

import numpy as np
import torch

import reverb_ref as ref
from sir_amd import synth

PART = 512
MAX_RIR_LENS = [PART * p for p in range(1, 17)] + [1, 513, 8191]
CASES = [(m, False) for m in MAX_RIR_LENS] + [(PART * p, True) for p in (1, 7, 16)]      # (max_rir_len, PCM16 input)
N_WAVES = 8


def case_id(c):
    return f"{c[0]}{'-pcm16' if c[1] else ''}"


def parts_of(max_rir_len):
    return (max_rir_len + PART - 1) // PART


def max_len_of(max_rir_len):
    return PART * (2 * (parts_of(max_rir_len) + 3) + 5)


@functools.lru_cache(maxsize=None)
def _master():
    flat = (0.2 * np.random.default_rng(77).standard_normal(8192)).astype(np.float32)
    flat[0] = 1.0
    x = synth.synth_clips(N_WAVES, max_len_of(8192), seed=41)
    return flat, x, synth.to_int16(x)


@functools.lru_cache(maxsize=None)
def ring_case(max_rir_len, pcm16=False):
    """-> dict: parts, ring, max_len, rirs (list of float32 arrays), names (of the RIRs), rows [(waveform, RIR or -1, length)],
    wave [rows][max_len] (float32 or int16, row b holding its waveform), x64 (the same as float64, PCM16 dequantised)"""
    flat, x32, x16 = _master()
    parts, max_len = parts_of(max_rir_len), max_len_of(max_rir_len)
    blocks = max_len // PART
    sign = 1.0 if parts % 2 else -1.0
    k_lone, k_short = PART * (parts - 1) + 1, PART * (parts - 1)
    lone = flat[:k_lone].copy()
    lone[-1] = 0.5 * sign
    decay = synth.synthetic_rir((max_rir_len + 0.5) / 16000.0, sample_rate=16000, rng=np.random.default_rng(100 + max_rir_len),
                                max_taps=max_rir_len).numpy()
    assert len(decay) == max_rir_len
    if max_rir_len > 1:
        decay[-1] = -0.5 * sign
    rirs, names = [flat[:max_rir_len], lone, decay, flat[:1]], ["flat", "lone", "decay", "one"]
    rows = [(0, 0, max_len), (1, 1, max_len - 7), (2, 2, max_len - 511), (3, 3, max_len - PART), (4, 0, PART * (blocks - 2) - 100),
            (5, 1, PART * (blocks - 3) - 37), (6, -1, max_len - 1000)]
    if k_short >= 1:
        rirs.append(flat[:k_short])
        names.append("short")
        rows.append((0, 4, max_len_of(k_short)))
    src = x16 if pcm16 else x32
    wave = torch.stack([src[w, :max_len] for w, _, _ in rows])
    return {"max_rir_len": max_rir_len, "parts": parts, "ring": parts + 3, "max_len": max_len, "rirs": rirs, "names": names, "rows": rows,
            "wave": wave, "x64": wave.double().numpy() / (32768.0 if pcm16 else 1.0)}


@functools.lru_cache(maxsize=None)
def oracle(max_rir_len, pcm16=False):
    """-> per row (y float64 [L], the bound |x|_inf |h|_1); computed once per case"""
    c = ring_case(max_rir_len, pcm16)
    res = []
    for b, (_, r, n) in enumerate(c["rows"]):
        x = c["x64"][b, :n]
        h = c["rirs"][r] if r >= 0 else None
        res.append((ref.reverb(x, h), np.abs(x).max() * (np.abs(h.astype(np.float64)).sum() if r >= 0 else 1.0)))
    return res
