"""Live streams: segment audio that arrives piece by piece on the GPU (host side of ``sir_stream_push`` / ``sir_stream_gather``).

``StreamSegmenter`` is the incremental form of ``sir_amd.segmenter.Segmenter``: ``n_streams`` independent sources -- callers of a
speech server, microphones -- each hand over a few samples per ``push``, the way the reference's ``MicrophoneListener.listen``
(scripts/testing.py:63-133) reads 1024 samples at a time, and every push returns the utterances it completed as a zero-tailed
clip batch.  The detector's state and a ring of recent samples per stream stay on the GPU between pushes.  The contract is in
include/sir_hip.h and DESIGN.md section 4; what a stream yields does not depend on how its samples were cut into pushes.

``StreamInput`` is the stage in front for streams that do not arrive as PCM at the detector's rate -- 8 kHz G.711 telephony first of
all: it decodes and rate-converts every stream push by push on the GPU (``sir_stream_input_push``) with a small carried filter
state, bit for bit ``sir_resample`` of the whole decoded stream.  ``StreamSegmenter(..., input_rate=, encoding=)`` owns one.
"""
import ctypes as C
import math

import torch

from . import _native, wave_args
from .segmenter import Segmenter

MAX_STREAMS = 65535
MAX_PUSH = 1 << 24
MAX_CHUNKS = 1 << 20
ENCODINGS = ("pcm", "ulaw", "alaw")
LOWPASS_FILTER_WIDTH, ROLLOFF = 6, 0.99          # sir_resample's filter (csrc/frontend.hip)


def _stream_mask(which, n_streams, device, what):
    """None, a [n_streams] bool / uint8 tensor or a sequence of stream indices -> uint8 [n_streams] on the device (or None)"""
    if which is None:
        return None
    if torch.is_tensor(which) and which.dtype in (torch.bool, torch.uint8):
        if which.numel() != n_streams:
            raise _native.SirError(f"{what} must hold one entry per stream: {which.numel()} for {n_streams}")
        return which.to(device=device, dtype=torch.uint8).contiguous()
    idx = [int(i) for i in which]
    if not idx:
        return None
    if min(idx) < 0 or max(idx) >= n_streams:
        raise _native.SirError(f"{what}: stream index outside [0, {n_streams})")
    mask = torch.zeros((n_streams,), dtype=torch.uint8)
    mask[idx] = 1
    return mask.to(device)


def input_dtype(encoding, dtype, pcm_default=torch.int16):
    """The dtype of a stream's pushes: ``dtype=None`` is ``pcm_default`` for "pcm" and uint8 for G.711; G.711 pushes are uint8 and
    nothing else is, anything that contradicts that raises ``ValueError``.  -> (torch dtype, SIR_WAVE_* code)."""
    if encoding not in ENCODINGS:
        raise ValueError(f"unknown stream encoding {encoding!r}: one of {ENCODINGS}")
    if encoding == "pcm":
        dtype = pcm_default if dtype is None else dtype
        code = wave_args.WAVE_CODES.get(dtype)
        if code is None:
            raise ValueError(f"unsupported stream dtype {dtype!r} for encoding 'pcm': int16 or float32")
        return dtype, code
    if dtype not in (None, torch.uint8):
        raise ValueError(f"a {encoding!r} stream is pushed as uint8 codes, not {dtype!r}")
    return torch.uint8, _native.WAVE_ULAW if encoding == "ulaw" else _native.WAVE_ALAW


def _push_args(owner, who, samples, lengths):
    """One push of ``owner`` (a ``StreamInput``, or a ``StreamSegmenter`` without one), checked: -> (samples, columns, lengths).
    ``samples=None`` brings nothing."""
    if samples is None:
        samples, lengths = owner._nothing, torch.zeros((owner.n_streams,), dtype=torch.int32, device=owner.device)
    must = f"samples must be {owner.dtype} [{owner.n_streams}, <= {owner.max_push}]"
    _, _, width, lengths = wave_args.check_batch(who, samples, lengths, "stream", must=must, rows=owner.n_streams,
                                                 dtypes={owner.dtype: owner.wave_dtype})
    if not 1 <= width <= owner.max_push:
        raise _native.SirError(f"a push brings 1 .. {owner.max_push} columns, got {width}")
    return samples, width, lengths


class StreamInput:
    """Decode and rate-convert live streams on the GPU, push by push (host side of ``sir_stream_input_push``): the thin owner of
    the per-stream filter state.  What a stream yields over its life is bit for bit ``HipFeaturizer.resample`` of the whole
    decoded stream, however it was cut into pushes (include/sir_hip.h, DESIGN.md section 4 "Stream input")."""

    def __init__(self, n_streams, max_push, input_rate, output_rate=16000, encoding="pcm", dtype=None, device=None):
        """``n_streams`` slots that receive at most ``max_push`` samples per push at ``input_rate`` Hz and yield float32 at
        ``output_rate`` Hz.  ``encoding``: "pcm" (``dtype`` int16, the default, or float32), "ulaw" or "alaw" (G.711, pushes are
        ``torch.uint8``).  Needs no GPU until the first ``push`` / ``reset``."""
        if int(n_streams) != n_streams or not 1 <= n_streams <= MAX_STREAMS:
            raise ValueError(f"n_streams must be an integer in [1, {MAX_STREAMS}], got {n_streams!r}")
        if int(max_push) != max_push or not 1 <= max_push <= MAX_PUSH:
            raise ValueError(f"max_push must be an integer in [1, {MAX_PUSH}], got {max_push!r}")
        for name, rate in (("input_rate", input_rate), ("output_rate", output_rate)):
            if isinstance(rate, bool) or int(rate) != rate or not 0 < rate < 1 << 31:
                raise ValueError(f"{name} must be a positive integer number of Hz, got {rate!r}")
        self.dtype, self.wave_dtype = input_dtype(encoding, dtype)
        self.encoding = encoding
        self.n_streams, self.max_push = int(n_streams), int(max_push)
        self.input_rate, self.output_rate = int(input_rate), int(output_rate)
        g = math.gcd(self.input_rate, self.output_rate)
        self.orig, self.new = self.input_rate // g, self.output_rate // g
        if self.orig == self.new:
            self.width, self.max_out = 0, self.max_push
        else:
            # sir_stream_input_max_out: ceil(new (max_push + 3 width + 2 orig) / orig) + 1
            self.width = math.ceil(LOWPASS_FILTER_WIDTH * self.orig / (min(self.orig, self.new) * ROLLOFF))
            self.max_out = -((-self.new * (self.max_push + 3 * self.width + 2 * self.orig)) // self.orig) + 1
        if self.max_out > 0x7FFFFFFF:
            raise ValueError(f"a push of {max_push} samples at {input_rate} -> {output_rate} Hz can emit {self.max_out} samples: "
                             "that does not fit an int32 length")
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self._state = None

    def config(self):
        return _native.StreamInputConfig(self.n_streams, self.wave_dtype, self.input_rate, self.output_rate, self.max_push)

    def _ensure(self):
        """allocate the state buffer on first use and zero the counters (the first use of a rate pair builds its filter table)"""
        if self._state is not None:
            return
        from .featurizer import get_featurizer
        lib = _native.lib()
        self._handle = get_featurizer().handle
        self._cfg = self.config()
        need = lib.sir_stream_input_state_bytes(self._handle, C.byref(self._cfg))
        if need == 0 or lib.sir_stream_input_max_out(C.byref(self._cfg)) != self.max_out:
            raise _native.SirError("unsupported stream input configuration")
        with torch.cuda.device(self.device):
            state = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._nothing = torch.zeros((self.n_streams, 16), dtype=self.dtype, device=self.device)
            rc = lib.sir_stream_input_reset(self._handle, state.data_ptr(), state.numel(), C.byref(self._cfg), None,
                                            _native.current_stream_ptr())
        _native.check(rc, "sir_stream_input_reset")
        self._state = state

    def reset(self, mask=None):
        """Forget the filter state of the streams in ``mask`` (a [n_streams] bool / uint8 tensor or stream indices; None = all)."""
        self._ensure()
        m = _stream_mask(mask, self.n_streams, self.device, "mask")
        rc = _native.lib().sir_stream_input_reset(self._handle, self._state.data_ptr(), self._state.numel(), C.byref(self._cfg),
                                                  m.data_ptr() if m is not None else None, _native.current_stream_ptr())
        _native.check(rc, "sir_stream_input_reset")

    def push(self, samples, lengths=None, close=None, out=None):
        """samples: [n_streams, <= max_push] of the input dtype on the GPU, row s = the new samples of stream s (None: nothing, a
        pure close); lengths: int32 [n_streams] on the GPU (default: every row is full).  ``close``: the streams that end with
        this push -- they emit their tail and the slot starts again at position 0.
        -> (out float32 [n_streams, max_out], out_lengths int32 [n_streams]); columns behind a row's length are not written.
        No host synchronisation.  ``out``: a float32 [n_streams, >= max_out] tensor to write into instead of a new one."""
        self._ensure()
        samples, width, lengths = _push_args(self, "StreamInput.push", samples, lengths)
        close = _stream_mask(close, self.n_streams, self.device, "close")
        out = wave_args.check_out(out, self.n_streams, self.max_out, self.device, f"[{self.n_streams}, >= {self.max_out}]")
        out_len = torch.empty((self.n_streams,), dtype=torch.int32, device=self.device)
        rc = _native.lib().sir_stream_input_push(self._handle, self._state.data_ptr(), self._state.numel(), C.byref(self._cfg),
                                                 samples.data_ptr(), samples.stride(0), width, lengths.data_ptr(),
                                                 close.data_ptr() if close is not None else None, out.data_ptr(), out.stride(0),
                                                 out_len.data_ptr(), _native.current_stream_ptr())
        _native.check(rc, "sir_stream_input_push")
        return out, out_len


class StreamSegmenter:
    def __init__(self, n_streams, max_push, max_utterance=10.0, dtype=None, device=None, sample_rate=16000, chunk_size=1024,
                 threshold=0.01, silence_limit=1, prior_recording=0.5, flush_tail=True, max_utt_chunks=None, ring_chunks=None,
                 input_rate=None, encoding=None):
        """``n_streams`` slots, at most ``max_push`` samples per slot and push, pushes of ``dtype`` (int16, the default, or
        float32).  An utterance that reaches ``max_utterance`` seconds is ended there (``forced``) so that the ring can be finite;
        the other arguments are ``Segmenter``'s, i.e. the listener's.  ``max_utt_chunks`` / ``ring_chunks`` override the chunk
        counts derived from ``max_utterance`` and the smallest legal ring.
        ``input_rate`` (Hz, default ``sample_rate``) / ``encoding`` ("pcm", "ulaw", "alaw"; default "pcm"): with either given the
        segmenter owns a ``StreamInput`` in front -- pushes arrive at ``input_rate`` in the input dtype (uint8 for G.711),
        ``max_push`` counts input samples, the detector and its ring run on the converted float32 samples, and table positions
        stay in ``sample_rate`` samples.  With neither the object launches exactly what it did without them.
        Needs no GPU until the first ``push`` / ``reset``."""
        if int(n_streams) != n_streams or not 1 <= n_streams <= MAX_STREAMS:
            raise ValueError(f"n_streams must be an integer in [1, {MAX_STREAMS}], got {n_streams!r}")
        if int(max_push) != max_push or not 1 <= max_push <= MAX_PUSH:
            raise ValueError(f"max_push must be an integer in [1, {MAX_PUSH}], got {max_push!r}")
        self.input = None
        inner_max_push = int(max_push)
        if input_rate is None and encoding is None:
            dtype, self.wave_dtype = input_dtype("pcm", dtype)
        else:
            self.input = StreamInput(n_streams, max_push, sample_rate if input_rate is None else input_rate, sample_rate,
                                     "pcm" if encoding is None else encoding, dtype, device)
            dtype, self.wave_dtype = self.input.dtype, _native.WAVE_F32
            inner_max_push = self.input.max_out
            if inner_max_push > MAX_PUSH:
                raise ValueError(f"a push of {max_push} samples becomes up to {inner_max_push} at {sample_rate} Hz: above {MAX_PUSH}")
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
        self._inner_max_push = inner_max_push                     # what one sir_stream_push may bring: the front stage's max_out
        self.chunks_per_push = -(-inner_max_push // self.chunk_size)
        self.min_ring_chunks = self.max_utt_chunks + self.chunks_per_push + 2
        self.ring_chunks = self.min_ring_chunks if ring_chunks is None else int(ring_chunks)
        if self.ring_chunks < self.min_ring_chunks:
            raise ValueError(f"ring_chunks {ring_chunks!r} is below the minimum {self.min_ring_chunks}")
        self.max_rows = self.n_streams * (self.chunks_per_push + 2)
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self._state = None

    def config(self):
        vad = _native.VadConfig(self.chunk_size, self.threshold, self.silence_chunks, self.prior_chunks, int(self.flush_tail))
        return _native.StreamConfig(vad, self.n_streams, self.wave_dtype, self._inner_max_push, self.max_utt_chunks, self.ring_chunks)

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
            if self.input is not None:                            # the front stage's output, consumed by the push queued behind it
                self.input._ensure()
                self._converted = torch.zeros((self.n_streams, self.input.max_out), dtype=torch.float32, device=self.device)
            rc = lib.sir_stream_reset(self._handle, state.data_ptr(), state.numel(), C.byref(self._cfg), None, _native.current_stream_ptr())
        _native.check(rc, "sir_stream_reset")
        self._state = state

    def _mask(self, which, what):
        return _stream_mask(which, self.n_streams, self.device, what)

    def reset(self, mask=None):
        """Forget the state of the streams in ``mask`` (see ``push``'s ``close`` for its forms; None = all)."""
        self._ensure()
        m = self._mask(mask, "mask")
        if self.input is not None:
            self.input.reset(m)
        rc = _native.lib().sir_stream_reset(self._handle, self._state.data_ptr(), self._state.numel(), C.byref(self._cfg),
                                            m.data_ptr() if m is not None else None, _native.current_stream_ptr())
        _native.check(rc, "sir_stream_reset")

    def push_table(self, samples, lengths=None, close=None, energy_out=None):
        """The segmenting half of ``push``: -> (table int64 [n, 4] = {stream, start, end, flags} on the GPU, stream-major then
        by time, positions in samples since the stream's last close; total int32 [1]).  ``total`` is read once -- the one host
        synchronisation.  The table is a copy: the next push does not change it.  ``samples=None`` brings nothing (a pure close).
        With a ``StreamInput`` in front, ``samples`` are in its dtype at ``input_rate``; ``close`` goes to both stages."""
        self._ensure()
        close = self._mask(close, "close")
        if energy_out is not None:
            _native.require_hip(energy_out)
            if energy_out.dtype != torch.float32 or not energy_out.is_contiguous() \
                    or tuple(energy_out.shape) != (self.n_streams, self.chunks_per_push + 1):
                raise _native.SirError("energy_out must be a contiguous float32 [n_streams, ceil(max_push / chunk_size) + 1] tensor")
        if self.input is not None:
            # decode and rate-convert first: what the detector is handed is float32 at sample_rate, at most max_out columns
            samples, lengths = self.input.push(samples, lengths, close, out=self._converted)
        else:
            samples, _, lengths = _push_args(self, "StreamSegmenter.push_table", samples, lengths)
        width = samples.shape[1]
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
        table, max_clip_len, out, out_len = wave_args.check_gather(table, total, max_clip_len, torch.int64, 4, self.device)
        n = table.shape[0]
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
