"""Utterance segmentation of long recordings on the GPU (host side of ``sir_vad_segment`` / ``sir_vad_gather``).

``Segmenter`` is the batch form of the reference's ``MicrophoneListener`` (scripts/testing.py:19-133) with the listener's
argument names: instead of cutting one live stream into utterances chunk by chunk, it finds the utterances of many recordings
resident in HBM in one launch sequence and hands them on as a zero-tailed clip batch -- what ``HipFeaturizer`` and the ragged
forward take.  The contract (energy, trigger, prior buffer, silence limit, and the two deliberate differences from the listener)
is in include/sir_hip.h and DESIGN.md section 4.
"""
import ctypes as C
import math

import torch

from . import _native, wave_args

MIN_CHUNK, MAX_CHUNK = 64, 4096
WAVE_MUST = "wave must be [n_rec, L]"


class Segmenter:
    initial_seg_cap = 1024       # rows of the first segment table; it is regrown to the true total when that is larger

    def __init__(self, sample_rate=16000, chunk_size=1024, threshold=0.01, silence_limit=1, prior_recording=0.5, flush_tail=True):
        """Arguments as ``MicrophoneListener.__init__`` (testing.py:20-21) plus ``flush_tail``: emit (True) or drop (False, the
        listener's behaviour) an utterance still open where a recording stops.  Needs no GPU: the chunk counts are host
        arithmetic -- ``prior_chunks = int(prior_recording * sample_rate / chunk_size)`` (:63) and ``silence_chunks``, the
        first count at which the listener's ``silence_chunks * (chunk_size / sample_rate) >= silence_limit`` (:110-111) holds."""
        if int(sample_rate) != sample_rate or sample_rate <= 0:
            raise ValueError(f"sample_rate must be a positive integer, got {sample_rate!r}")
        if int(chunk_size) != chunk_size or not MIN_CHUNK <= chunk_size <= MAX_CHUNK or chunk_size % 64:
            raise ValueError(f"chunk_size must be a multiple of 64 in [{MIN_CHUNK}, {MAX_CHUNK}], got {chunk_size!r}")
        threshold = float(threshold)
        if math.isnan(threshold) or threshold < 0:
            raise ValueError(f"threshold must be >= 0, got {threshold!r}")
        silence_limit, prior_recording = float(silence_limit), float(prior_recording)
        if not (0 <= silence_limit < math.inf):
            raise ValueError(f"silence_limit must be a finite number of seconds >= 0, got {silence_limit!r}")
        if not (0 <= prior_recording < math.inf):
            raise ValueError(f"prior_recording must be a finite number of seconds >= 0, got {prior_recording!r}")
        self.sample_rate, self.chunk_size, self.threshold = int(sample_rate), int(chunk_size), threshold
        self.silence_limit, self.prior_recording, self.flush_tail = silence_limit, prior_recording, bool(flush_tail)
        self.prior_chunks = int(prior_recording * self.sample_rate / self.chunk_size)
        self.silence_chunks = _native.lib().sir_vad_stop_chunks(self.sample_rate, self.chunk_size, silence_limit)
        if self.silence_chunks < 0:
            raise ValueError(f"silence_limit {silence_limit!r} is out of range for chunks of {chunk_size} samples")
        self._scratch = wave_args.StreamScratch()
        self._seg_cap = 0

    def config(self):
        return _native.VadConfig(self.chunk_size, self.threshold, self.silence_chunks, self.prior_chunks, int(self.flush_tail))

    def segment(self, wave, lengths=None, energy_out=None):
        """wave: [n_rec, L] int16 or float32 on the GPU, lengths: int32 [n_rec] on the GPU (default: all L).
        -> (seg_table int32 [total, 3] = {recording, start sample, end sample}, recording-major then by time,
            seg_count int32 [n_rec], total int32 [1]), all on the GPU.
        ``total`` is read once -- the one host synchronisation; if the table was too small it is regrown and the call repeated.
        ``energy_out`` (test hook): float32 [n_rec, ceil(L / chunk_size)] receives the chunk energies."""
        from .featurizer import get_featurizer
        dt, n_rec, max_len, lengths = wave_args.check_batch("Segmenter.segment", wave, lengths, "recording", must=WAVE_MUST)
        dev = wave.device
        seg_count = torch.zeros((n_rec,), dtype=torch.int32, device=dev)
        total = torch.zeros((1,), dtype=torch.int32, device=dev)
        if n_rec == 0 or max_len == 0:
            return torch.zeros((0, 3), dtype=torch.int32, device=dev), seg_count, total
        lib = _native.lib()
        h = get_featurizer().handle
        if energy_out is not None:
            _native.require_hip(energy_out)
            if energy_out.dtype != torch.float32 or not energy_out.is_contiguous() \
                    or tuple(energy_out.shape) != (n_rec, -(-max_len // self.chunk_size)):
                raise _native.SirError("energy_out must be a contiguous float32 [n_rec, ceil(L / chunk_size)] tensor")
        need = lib.sir_vad_workspace_bytes(h, n_rec, max_len, self.chunk_size)
        if need == 0:
            raise _native.SirError(f"unsupported shape n_rec={n_rec} samples={max_len}")
        ws = self._scratch.get(need, dev)
        cfg = self.config()
        cap = max(self._seg_cap, self.initial_seg_cap)
        while True:
            table = torch.empty((cap, 3), dtype=torch.int32, device=dev)
            rc = lib.sir_vad_segment(h, wave.data_ptr(), dt, wave.stride(0), lengths.data_ptr(), n_rec, max_len, C.byref(cfg),
                                     energy_out.data_ptr() if energy_out is not None else None, seg_count.data_ptr(),
                                     table.data_ptr(), cap, total.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _native.current_stream_ptr())
            _native.check(rc, "sir_vad_segment")
            n = int(total.item())
            if n <= cap:
                break
            cap = n
        self._seg_cap = cap
        return table[:n], seg_count, total

    def gather(self, wave, table, total, max_clip_len):
        """Cut the rows of a ``segment`` result out of ``wave``: -> (clips float32 [n, max_clip_len], zero behind each clip's
        length, clip_lengths int32 [n]).  int16 is dequantised as s / 32768; a segment longer than ``max_clip_len`` samples is
        cut there.  A table row outside the batch gives a zero row and ``ops.check_status()`` raises."""
        from .featurizer import get_featurizer
        _native.require_hip(wave)
        dt = wave_args.check_wave("Segmenter.gather", wave, WAVE_MUST)[0]
        table, max_clip_len, out, out_len = wave_args.check_gather(table, total, max_clip_len, torch.int32, 3, wave.device)
        n = table.shape[0]
        if n == 0:
            return out, out_len
        rc = _native.lib().sir_vad_gather(get_featurizer().handle, wave.data_ptr(), dt, wave.stride(0), wave.shape[0], table.data_ptr(),
                                          total.data_ptr(), n, out.data_ptr(), out.stride(0), max_clip_len, out_len.data_ptr(),
                                          _native.current_stream_ptr())
        _native.check(rc, "sir_vad_gather")
        return out, out_len

    def clips(self, wave, lengths=None, max_clip_len=None):
        """``segment`` then ``gather``: -> (clips, clip_lengths, seg_table).  ``max_clip_len`` defaults to the longest segment
        found (one more small copy to the host)."""
        table, _, total = self.segment(wave, lengths)
        if max_clip_len is None:
            max_clip_len = int((table[:, 2] - table[:, 1]).max().item()) if table.shape[0] else 1
        out, out_len = self.gather(wave, table, total, max_clip_len)
        return out, out_len, table
