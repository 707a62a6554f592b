"""Host reference of the live-stream segmenter (``sir_stream_push`` / ``sir_stream_gather``), plain numpy, built on tests/vad_ref.py.

``StreamRef`` is one stream: the listener's loop of ``vad_ref.segments_loop`` with its state carried from push to push, the forced
cut at ``max_utt_chunks`` and the close of include/sir_hip.h.  Rows are ``(start sample, end sample, flags)``; positions count
from the stream's last close.  Energies are formed in float64 by ``vad_ref.chunk_energy``; ``flags=`` replaces them by a given
vector of decisions (chunk i of the stream's current life -> ``flags[i]``), for tests of the state machine alone.
"""
import numpy as np

import vad_ref

FORCED, FLUSHED = 1, 2


class StreamRef:
    def __init__(self, c, threshold, prior_chunks, silence_chunks, max_utt_chunks, flush_tail=True, flags=None):
        assert max_utt_chunks > prior_chunks
        self.c, self.threshold, self.P, self.n_stop, self.M = c, threshold, prior_chunks, silence_chunks, max_utt_chunks
        self.flush_tail, self.flags = flush_tail, flags
        self._zero()

    def _zero(self):
        self.n = self.j = self.silence = self.first = 0
        self.recording = False
        self.samples = []                        # everything since the last close, for gather()

    def wave(self):
        return np.concatenate(self.samples) if self.samples else np.zeros(0, dtype=np.float32)

    def _speech(self, i, x):
        if self.flags is not None:
            return bool(self.flags[i])
        e = vad_ref.chunk_energy(x, len(x), self.c)[0]
        return bool(np.float32(e) > np.float32(self.threshold))

    def _judge(self, i, speech, rows):
        if not self.recording and speech:
            self.recording, self.silence = True, 0
            self.first = max(0, i - self.P + 1) if self.P >= 1 else i
        if self.recording:
            self.silence = 0 if speech else self.silence + 1
            flag = 0 if self.silence >= self.n_stop else (FORCED if i - self.first + 1 >= self.M else None)
            if flag is not None:
                rows.append((self.first * self.c, min((i + 1) * self.c, self.n), flag))
                self.recording = False

    def push(self, x, close=False):
        """append x, judge every chunk it completes -> the rows that ended, in time order"""
        x = np.asarray(x)
        rows = []
        if len(x):
            self.samples.append(x)
            self.n += len(x)
        w = self.wave() if (self.n // self.c > self.j or close) else None
        while (self.j + 1) * self.c <= self.n:
            self._judge(self.j, self._speech(self.j, w[self.j * self.c:(self.j + 1) * self.c]), rows)
            self.j += 1
        if close:
            if self.n % self.c:
                self._judge(self.j, self._speech(self.j, w[self.j * self.c:]), rows)
            if self.recording and self.flush_tail:
                rows.append((self.first * self.c, self.n, FLUSHED))
            self._zero()
        return rows


def run(x, pieces, c, threshold, prior_chunks, silence_chunks, max_utt_chunks, flush_tail=True, flags=None):
    """one recording fed in pushes of ``pieces`` samples (a sequence that sums to len(x)), closed with its last sample"""
    ref = StreamRef(c, threshold, prior_chunks, silence_chunks, max_utt_chunks, flush_tail, flags)
    assert sum(pieces) == len(x)
    rows, at = [], 0
    for k, m in enumerate(pieces):
        rows += ref.push(x[at:at + m], close=(k == len(pieces) - 1))
        at += m
    if not len(pieces):
        rows += ref.push(x[:0], close=True)
    return rows


def gather(x, rows, max_clip_len):
    """-> (clips float32 [n, max_clip_len], lengths int32 [n]) of the rows of one stream cut out of its samples x"""
    table = [(0, a, b) for a, b, _ in rows]
    return vad_ref.gather([np.asarray(x)], table, max_clip_len)
