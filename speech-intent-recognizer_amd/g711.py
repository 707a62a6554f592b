"""G.711 (ITU-T): the two 256-entry expansion tables, byte code -> 16-bit linear value, and a nearest-value encoder.

Host side of telephony audio.  ``scripts/utils/wav_io.read_wav`` decodes WAVE format tags 7 (mu-law) and 6 (A-law) through these
tables; a live stream is NOT decoded on the host -- ``sir_stream_input_push`` expands the bytes on the GPU with the same closed
forms (include/sir_hip.h), and ``x = v / 32768`` is exact in float32 either way.

    mu-law  u = ~b & 0xFF, t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7), v = 0x84 - t if u & 0x80 else t - 0x84
    A-law   a = b ^ 0x55, e = (a >> 4) & 7, m = a & 0x0F, t = ((m << 4) + 0x108) << (e - 1) if e else (m << 4) + 8,
            v = t if a & 0x80 else -t
"""
import numpy as np

LAWS = ("ulaw", "alaw")


def _ulaw_table():
    u = ~np.arange(256, dtype=np.int32) & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int16)


def _alaw_table():
    a = np.arange(256, dtype=np.int32) ^ 0x55
    e, m = (a >> 4) & 7, a & 0x0F
    t = np.where(e > 0, ((m << 4) + 0x108) << np.maximum(e - 1, 0), (m << 4) + 8)
    return np.where(a & 0x80, t, -t).astype(np.int16)


ULAW_TABLE = _ulaw_table()       # int16 [256]: 0xFF, 0x7F -> 0; 0x80 -> +32124; 0x00 -> -32124
ALAW_TABLE = _alaw_table()       # int16 [256]: 0xD5 -> +8; 0x55 -> -8; 0xAA -> +32256; 0x2A -> -32256
ULAW_TABLE.setflags(write=False)
ALAW_TABLE.setflags(write=False)


def table(law):
    if law not in LAWS:
        raise ValueError(f"unknown G.711 law {law!r}: 'ulaw' or 'alaw'")
    return ULAW_TABLE if law == "ulaw" else ALAW_TABLE


def decode(codes, law):
    """uint8 codes (any shape) -> int16 linear values."""
    codes = np.asarray(codes)
    if codes.dtype != np.uint8:
        raise ValueError(f"G.711 codes are uint8, got {codes.dtype}")
    return table(law)[codes]


def encode(pcm16, law):
    """int16 linear values (any shape) -> the uint8 code whose expansion is nearest (ties: the smaller value).  Not the bit-exact
    ITU compressor -- it serves tests and tools that need some valid code stream for a given signal."""
    tab = table(law).astype(np.int32)
    order = np.argsort(tab, kind="stable")
    vals = tab[order]
    x = np.asarray(pcm16).astype(np.int32)
    hi = np.clip(np.searchsorted(vals, x, side="left"), 0, 255)
    lo = np.clip(hi - 1, 0, 255)
    pick = np.where(np.abs(vals[lo] - x) <= np.abs(vals[hi] - x), lo, hi)
    return order[pick].astype(np.uint8)
