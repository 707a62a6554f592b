"""Live streams: segment audio that arrives piece by piece on the GPU (host side of ``sir_stream_push`` / ``sir_stream_gather``).

``StreamSegmenter`` is the incremental form of ``sir_amd.segmenter.Segmenter``: ``n_streams`` independent sources -- callers of a
speech server, microphones -- each hand over a few samples per ``push``, the way the reference's ``MicrophoneListener.listen``
(scripts/testing.py:63-133) reads 1024 samples at a time, and every push returns the utterances it completed as a zero-tailed
clip batch.  The detector's state and a ring of recent samples per stream stay on the GPU between pushes.  The contract is in
include/sir_hip.h and DESIGN.md section 4; what a stream yields does not depend on how its samples were cut into pushes.
"""
import ctypes as C
import math

import torch

from . import _native
from .segmenter import Segmenter

MAX_STREAMS = 65535
MAX_PUSH = 1 << 24
MAX_CHUNKS = 1 << 20


class StreamSegmenter:
    def __init__(self, n_streams, max_push, max_utterance=10.0, dtype=torch.int16, device=None, sample_rate=16000, chunk_size=1024,
                 threshold=0.01, silence_limit=1, prior_recording=0.5, flush_tail=True, max_utt_chunks=None, ring_chunks=None):
        """``n_streams`` slots, at most ``max_push`` samples per slot and push, pushes of ``dtype`` (int16 or float32).  An
        utterance that reaches ``max_utterance`` seconds is ended there (``forced``) so that the ring can be finite; the other
        arguments are ``Segmenter``'s, i.e. the listener's.  ``max_utt_chunks`` / ``ring_chunks`` override the chunk counts derived
        from ``max_utterance`` and the smallest legal ring.  Needs no GPU until the first ``push`` / ``reset``."""
        if int(n_streams) != n_streams or not 1 <= n_streams <= MAX_STREAMS:
            raise ValueError(f"n_streams must be an integer in [1, {MAX_STREAMS}], got {n_streams!r}")
        if int(max_push) != max_push or not 1 <= max_push <= MAX_PUSH:
            raise ValueError(f"max_push must be an integer in [1, {MAX_PUSH}], got {max_push!r}")
        self.wave_dtype = {torch.float32: _native.WAVE_F32, torch.int16: _native.WAVE_I16}.get(dtype)
        if self.wave_dtype is None:
            raise ValueError(f"unsupported stream dtype {dtype!r}: int16 or float32")
        seg = Segmenter(sample_rate, chunk_size, threshold, silence_limit, prior_recording, flush_tail)
        self.sample_rate, self.chunk_size, self.threshold = seg.sample_rate, seg.chunk_size, seg.threshold
        self.silence_chunks, self.prior_chunks, self.flush_tail = seg.silence_chunks, seg.prior_chunks, seg.flush_tail
        if max_utt_chunks is None:
            max_utterance = float(max_utterance)
            if not (0 < max_utterance < math.inf):
                raise ValueError(f"max_utterance must be a finite number of seconds > 0, got {max_utterance!r}")
            max_utt_chunks = math.ceil(max_utterance * self.sample_rate / self.chunk_size)
        if int(max_utt_chunks) != max_utt_chunks or not self.prior_chunks < max_utt_chunks <= MAX_CHUNKS:
            raise ValueError(f"an utterance may last {max_utt_chunks} chunks: it must be longer than the prior recording "
                             f"({self.prior_chunks} chunks) and at most {MAX_CHUNKS} chunks")
        self.n_streams, self.max_push, self.dtype, self.max_utt_chunks = int(n_streams), int(max_push), dtype, int(max_utt_chunks)
        self.chunks_per_push = -(-self.max_push // self.chunk_size)
        self.min_ring_chunks = self.max_utt_chunks + self.chunks_per_push + 2
        self.ring_chunks = self.min_ring_chunks if ring_chunks is None else int(ring_chunks)
        if self.ring_chunks < self.min_ring_chunks:
            raise ValueError(f"ring_chunks {ring_chunks!r} is below the minimum {self.min_ring_chunks}")
        self.max_rows = self.n_streams * (self.chunks_per_push + 2)
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self._state = None

    def config(self):
        vad = _native.VadConfig(self.chunk_size, self.threshold, self.silence_chunks, self.prior_chunks, int(self.flush_tail))
        return _native.StreamConfig(vad, self.n_streams, self.wave_dtype, self.max_push, self.max_utt_chunks, self.ring_chunks)

    def _ensure(self):
        """allocate the state buffer and the row table on first use, and zero the state"""
        if self._state is not None:
            return
        from .featurizer import get_featurizer
        lib = _native.lib()
        self._handle = get_featurizer().handle
        self._cfg = self.config()
        need = lib.sir_stream_state_bytes(self._handle, C.byref(self._cfg))
        if need == 0 or lib.sir_stream_max_rows(C.byref(self._cfg)) != self.max_rows:
            raise _native.SirError("unsupported stream configuration")
        with torch.cuda.device(self.device):
            state = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._table = torch.zeros((self.max_rows, 4), dtype=torch.int64, device=self.device)
            self._total = torch.zeros((1,), dtype=torch.int32, device=self.device)
            self._nothing = torch.zeros((self.n_streams, 8), dtype=self.dtype, device=self.device)
            rc = lib.sir_stream_reset(self._handle, state.data_ptr(), state.numel(), C.byref(self._cfg), None, _native.current_stream_ptr())
        _native.check(rc, "sir_stream_reset")
        self._state = state

    def _mask(self, which, what):
        """None, a [n_streams] bool / uint8 tensor or a sequence of stream indices -> uint8 [n_streams] on the device (or None)"""
        if which is None:
            return None
        if torch.is_tensor(which) and which.dtype in (torch.bool, torch.uint8):
            if which.numel() != self.n_streams:
                raise _native.SirError(f"{what} must hold one entry per stream: {which.numel()} for {self.n_streams}")
            return which.to(device=self.device, dtype=torch.uint8).contiguous()
        idx = [int(i) for i in which]
        if not idx:
            return None
        if min(idx) < 0 or max(idx) >= self.n_streams:
            raise _native.SirError(f"{what}: stream index outside [0, {self.n_streams})")
        mask = torch.zeros((self.n_streams,), dtype=torch.uint8)
        mask[idx] = 1
        return mask.to(self.device)

    def reset(self, mask=None):
        """Forget the state of the streams in ``mask`` (see ``push``'s ``close`` for its forms; None = all)."""
        self._ensure()
        m = self._mask(mask, "mask")
        rc = _native.lib().sir_stream_reset(self._handle, self._state.data_ptr(), self._state.numel(), C.byref(self._cfg),
                                            m.data_ptr() if m is not None else None, _native.current_stream_ptr())
        _native.check(rc, "sir_stream_reset")

    def push_table(self, samples, lengths=None, close=None, energy_out=None):
        """The segmenting half of ``push``: -> (table int64 [n, 4] = {stream, start, end, flags} on the GPU, stream-major then
        by time, positions in samples since the stream's last close; total int32 [1]).  ``total`` is read once -- the one host
        synchronisation.  The table is a copy: the next push does not change it.  ``samples=None`` brings nothing (a pure close)."""
        self._ensure()
        if samples is None:
            samples, lengths = self._nothing, torch.zeros((self.n_streams,), dtype=torch.int32, device=self.device)
        _native.require_hip(samples, lengths)
        if samples.dim() != 2 or samples.shape[0] != self.n_streams or samples.stride(1) != 1 or samples.dtype != self.dtype:
            raise _native.SirError(f"samples must be {self.dtype} [{self.n_streams}, <= {self.max_push}] with unit inner stride")
        width = samples.shape[1]
        if not 1 <= width <= self.max_push:
            raise _native.SirError(f"a push brings 1 .. {self.max_push} columns, got {width}")
        if lengths is None:
            lengths = torch.full((self.n_streams,), width, dtype=torch.int32, device=self.device)
        if lengths.numel() != self.n_streams:
            raise _native.SirError(f"lengths must hold one entry per stream: {lengths.numel()} for {self.n_streams}")
        lengths = lengths.to(torch.int32).contiguous()
        close = self._mask(close, "close")
        if energy_out is not None:
            _native.require_hip(energy_out)
            if energy_out.dtype != torch.float32 or not energy_out.is_contiguous() \
                    or tuple(energy_out.shape) != (self.n_streams, self.chunks_per_push + 1):
                raise _native.SirError("energy_out must be a contiguous float32 [n_streams, ceil(max_push / chunk_size) + 1] tensor")
        rc = _native.lib().sir_stream_push(self._handle, self._state.data_ptr(), self._state.numel(), C.byref(self._cfg), samples.data_ptr(),
                                           samples.stride(0), width, lengths.data_ptr(), close.data_ptr() if close is not None else None,
                                           energy_out.data_ptr() if energy_out is not None else None, self._table.data_ptr(),
                                           self.max_rows, self._total.data_ptr(), _native.current_stream_ptr())
        _native.check(rc, "sir_stream_push")
        n = int(self._total.item())
        return self._table[:n].clone(), self._total.clone()

    def gather(self, table, total, max_clip_len):
        """Cut the rows of the LATEST ``push_table`` out of the rings (the next push may overwrite them): -> (clips float32
        [n, max_clip_len], zero behind each clip's length, clip_lengths int32 [n]).  int16 is dequantised as s / 32768.  An
        impossible row gives a zero row and ``ops.check_status()`` raises."""
        self._ensure()
        _native.require_hip(table, total)
        max_clip_len = int(max_clip_len)
        if max_clip_len <= 0:
            raise _native.SirError(f"max_clip_len must be positive, got {max_clip_len}")
        if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 4 or total.dtype != torch.int32:
            raise _native.SirError("table must be int64 [n, 4] and total int32 [1]")
        table = table.contiguous()
        n = table.shape[0]
        out = torch.empty((n, max_clip_len), dtype=torch.float32, device=self.device)
        out_len = torch.empty((n,), dtype=torch.int32, device=self.device)
        if n == 0:
            return out, out_len
        rc = _native.lib().sir_stream_gather(self._handle, self._state.data_ptr(), self._state.numel(), C.byref(self._cfg), table.data_ptr(),
                                             total.data_ptr(), n, out.data_ptr(), out.stride(0), max_clip_len, out_len.data_ptr(),
                                             _native.current_stream_ptr())
        _native.check(rc, "sir_stream_gather")
        return out, out_len

    def push(self, samples, lengths=None, close=None, max_clip_len=None):
        """samples: [n_streams, <= max_push] of the stream dtype on the GPU, row s = the new samples of stream s; lengths: int32
        [n_streams] on the GPU (default: every row is full; 0 = nothing new for that stream).  ``close``: the streams that end with
        this push -- a [n_streams] bool / uint8 tensor or a sequence of indices; their trailing partial chunk is judged, an open
        utterance is flushed and the slot starts again at position 0.
        -> (clips, clip_lengths, table) of the utterances this push completed.  ``max_clip_len`` defaults to the longest of
        them (one more small copy to the host)."""
        table, total = self.push_table(samples, lengths, close)
        if max_clip_len is None:
            max_clip_len = int((table[:, 2] - table[:, 1]).max().item()) if table.shape[0] else 1
        out, out_len = self.gather(table, total, max(1, max_clip_len))
        return out, out_len, table
