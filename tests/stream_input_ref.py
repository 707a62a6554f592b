"""Host reference of the stream input stage (``sir_stream_input_push``, sir_amd.streaming.StreamInput) for
tests/test_stream_input_host.py and tests/test_stream_input_gpu.py.  Numpy only: no torch, no device.

* the two G.711 expanders in closed form (ITU-T G.711; include/sir_hip.h), independent of sir_amd/g711.py's tables;
* the emission rule: ``need(j)`` and ``E(n)`` from a polyphase table rebuilt with tests/frontend_edge_ref.py's definitions;
* the push schedules of the cut-invariance tests.

The output VALUES have no reference of their own here: the contract is bit-equality with ``sir_resample`` of the whole decoded
stream, and ``frontend_edge_ref.resample64`` / ``resample_bound`` hold that one to float64.
"""
import numpy as np

import frontend_edge_ref as fe

ANCHORS = {"ulaw": {0xFF: 0, 0x7F: 0, 0x80: 32124, 0x00: -32124}, "alaw": {0xD5: 8, 0x55: -8, 0xAA: 32256, 0x2A: -32256}}


# ---- decoding -----------------------------------------------------------------------------------------------------------------
def ulaw_expand(b):
    """mu-law byte(s) -> 16-bit linear value(s), int32."""
    u = ~np.asarray(b).astype(np.int32) & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int32)


def alaw_expand(b):
    """A-law byte(s) -> 16-bit linear value(s), int32."""
    a = np.asarray(b).astype(np.int32) ^ 0x55
    e, m = (a >> 4) & 7, a & 0x0F
    t = np.where(e > 0, ((m << 4) + 0x108) << np.maximum(e - 1, 0), (m << 4) + 8)
    return np.where(a & 0x80, t, -t).astype(np.int32)


def expand(b, law):
    return {"ulaw": ulaw_expand, "alaw": alaw_expand}[law](b)


def decode(x, encoding):
    """what the stage makes of a push row before it filters: float32, v / 32768 (exact) for codes and int16, float32 as it is"""
    x = np.asarray(x)
    if encoding in ("ulaw", "alaw"):
        assert x.dtype == np.uint8
        return (expand(x, encoding).astype(np.float64) / 32768.0).astype(np.float32)
    if x.dtype == np.int16:
        return (x.astype(np.float64) / 32768.0).astype(np.float32)
    assert x.dtype == np.float32
    return x


# ---- the emission rule -----------------------------------------------------------------------------------------------------------
class Table:
    """The shape of the polyphase table of a rate pair -- ``orig``, ``nw``, ``width``, per phase the index ``first[p]`` of the first
    in-window tap of the row of K = 2 width + orig taps, and the common chain length ``L`` (the longest in-window run) -- from
    frontend_edge_ref's definitions: ``width``, the float32 phase term and the ``|tt| < 6`` window test of ``h64``.
    This restates what csrc/frontend.hip's build_table keeps as ``first`` / ``L``; it evaluates no tap."""

    def __init__(self, orig_freq, new_freq):
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.orig, self.nw = fe.reduced(orig_freq, new_freq)
        self.width = fe.width(orig_freq, new_freq)
        self.K = 2 * self.width + self.orig
        base = min(self.orig, self.nw) * fe.ROLLOFF
        p = np.arange(self.nw, dtype=np.int64)
        phi = ((-p).astype(np.float32) / np.float32(self.nw)).astype(np.float64)
        k = np.arange(self.K, dtype=np.int64)
        tt = (phi[:, None] + (k[None, :] - self.width) / self.orig) * base
        inside = np.abs(tt) < fe.LOWPASS_FILTER_WIDTH
        assert inside.any(axis=1).all()
        self.first = inside.argmax(axis=1).astype(np.int64)
        last = self.K - 1 - inside[:, ::-1].argmax(axis=1)
        self.L = int((last - self.first + 1).max())

    def need(self, j):
        """input samples output j needs: q orig + first[p] - width + L."""
        j = np.asarray(j, dtype=np.int64)
        return (j // self.nw) * self.orig + self.first[j % self.nw] - self.width + self.L

    def emitted(self, n):
        """E(n): the largest J with need(j) <= n for all j < J -- a plain walk from j = 0, nothing assumed about need's order."""
        j = 0
        while int(self.need(j)) <= n:
            j += 1
        return j

    def emitted_upto(self, n_max):
        """E(n) for n = 0 .. n_max as an int64 array (one walk)."""
        out = np.zeros(n_max + 1, dtype=np.int64)
        j = 0
        for n in range(n_max + 1):
            while int(self.need(j)) <= n:
                j += 1
            out[n] = j
        return out

    def out_len(self, n):
        return fe.out_len(n, self.orig_freq, self.new_freq)

    def max_out(self, max_in):
        """sir_stream_input_max_out: ceil(nw (max_in + 3 width + 2 orig) / orig) + 1."""
        return -((-self.nw * (max_in + 3 * self.width + 2 * self.orig)) // self.orig) + 1

    def stream_length(self):
        """N = 2 (2 width + orig) + 37: the stream of the cut-invariance cases."""
        return 2 * self.K + 37


def counts(table, pieces, close_last=True):
    """per push of ``pieces`` samples the number of outputs it must emit: E(n_after) - E(n_before), the closing push up to
    out_len(n); a push of nothing that does not close emits nothing"""
    n, e, out = 0, 0, []
    E = table.emitted_upto(sum(pieces))
    for k, m in enumerate(pieces):
        n += m
        closing = close_last and k == len(pieces) - 1
        e1 = table.out_len(n) if closing else (int(E[n]) if m else e)
        out.append(e1 - e)
        e = e1
    return out


# ---- push schedules ------------------------------------------------------------------------------------------------------------
def _split(total, most):
    return [most] * (total // most) + ([total % most] if total % most else [])


def _from_cuts(cuts, total, most):
    """ascending cut points -> piece sizes, no piece above ``most``"""
    pts = [0] + sorted({c for c in cuts if 0 < c < total}) + [total]
    out = []
    for a, b in zip(pts[:-1], pts[1:]):
        out += _split(b - a, most)
    return out


def schedules(table, total, max_in, seed=0):
    """-> {name: piece sizes that sum to ``total``, each <= max_in}: one sample per push; max_in per push; seeded random cuts
    (0 .. max_in, empty pushes included); cuts exactly at, one before and one after need(j) of the first 2 nw outputs.  The fifth
    schedule of the tests, one push of everything, needs max_in >= total and is built by the caller."""
    rng = np.random.default_rng(seed)
    rand, left = [], total
    while left > 0:
        m = min(left, int(rng.integers(0, max_in + 1)))
        rand.append(m)
        left -= m
    edges = []
    for j in range(2 * table.nw):
        nj = int(table.need(j))
        edges += [nj - 1, nj, nj + 1]
    out = {"one": [1] * total, "max": _split(total, max_in), "random": rand, "need_edges": _from_cuts(edges, total, max_in)}
    assert all(sum(p) == total and max(p) <= max_in for p in out.values())
    return out
