"""CPU: the live-stream segmenter's reference (tests/stream_ref.py) against the batch reference (tests/vad_ref.py) and on the
hand-worked forced-cut case, the library's new symbols and size helpers, and ``StreamSegmenter``'s argument handling.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import stream_ref
import vad_ref
from sir_amd import _native
from sir_amd.streaming import StreamSegmenter

C = 64
NAMES = ["sir_stream_min_ring_chunks", "sir_stream_max_rows", "sir_stream_state_bytes", "sir_stream_reset", "sir_stream_push",
         "sir_stream_gather"]


def _pieces(rng, total, most):
    """a random cut of `total` samples into pushes of 0 .. most samples"""
    out = []
    while total > 0:
        m = min(total, int(rng.integers(0, most + 1)))
        out.append(m)
        total -= m
    return out


def _cfg(c=C, thr=0.01, n_stop=2, prior=3, flush=1, S=4, dtype=_native.WAVE_I16, max_in=200, M=12, R=18):
    return _native.StreamConfig(_native.VadConfig(c, thr, n_stop, prior, flush), S, dtype, max_in, M, R)


def test_library_exports_the_stream_symbols():
    if not _native.os.path.exists(_native.LIB_PATH):
        _native.build()
    handle = ctypes.CDLL(_native.LIB_PATH)
    for n in NAMES:
        assert hasattr(handle, n), f"{n} is not exported"
        assert n in _native.SIGNATURES
    assert ctypes.sizeof(_native.StreamConfig) == 40
    assert (_native.STREAM_FORCED, _native.STREAM_FLUSHED) == (stream_ref.FORCED, stream_ref.FLUSHED) == (1, 2)


def test_random_pieces_equal_the_batch_reference_when_nothing_is_forced():
    """2 000 random flag vectors, each fed in random pieces (0 .. 3 chunks and a bit per push) and closed with its last sample:
    the rows are the batch form's with flush_tail, whatever the cut"""
    rng = np.random.default_rng(20241019)
    n_cases = 0
    for density in (0.05, 0.2, 0.5, 0.9):
        for _ in range(500):
            n = int(rng.integers(1, 61))
            f = rng.random(n) < density
            P, n_stop = int(rng.integers(0, 5)), int(rng.integers(0, 5))
            length = n * C - int(rng.integers(0, C))
            flush = bool(rng.integers(0, 2))
            want = vad_ref.segments_loop(f, length, C, P, n_stop, flush)
            x = np.zeros(length, dtype=np.int16)
            for most in (1000000, 3 * C + 5):
                got = stream_ref.run(x, _pieces(rng, length, min(most, length)), C, 0.01, P, n_stop, 1 << 20, flush, flags=f)
                assert [(a, b) for a, b, _ in got] == want, (f.astype(int).tolist(), length, P, n_stop, flush)
                assert all(fl == 0 for _, _, fl in got[:-1])
                if got and got[-1][2]:                      # only the last row can be the flush, and only of an open utterance
                    assert got[-1][2] == stream_ref.FLUSHED and flush and got[-1][1] == length
            n_cases += 1
    assert n_cases == 2000


def test_forced_cut_of_a_continuously_loud_input():
    # c 64, P 3, n_stop 2, M 12, 40 loud chunks: the utterance triggered at chunk 0 is cut at chunk 11; chunk 12 triggers the next
    # one, whose prior buffer reaches back to chunk 10 -- inside the previous utterance -- and so on; the last one is open at the close
    F, L = stream_ref.FORCED, stream_ref.FLUSHED
    want = [(0, 768, F), (640, 1408, F), (1280, 2048, F), (1920, 2560, L)]
    x = np.full(40 * C, 8000, dtype=np.int16)
    rng = np.random.default_rng(3)
    for pieces in ([40 * C], [C] * 40, [1000, 1000, 560], _pieces(rng, 40 * C, 200), _pieces(rng, 40 * C, 63)):
        assert stream_ref.run(x, pieces, C, 0.01, 3, 2, 12) == want
    assert stream_ref.run(x, [40 * C], C, 0.01, 3, 2, 12, flush_tail=False) == want[:3]
    # the reference alone: silence ends an utterance before the cut can
    x[5 * C:] = 0
    assert stream_ref.run(x, [1000, 1000, 560], C, 0.01, 3, 2, 12) == [(0, 7 * C, 0)]


def test_close_judges_the_partial_chunk_and_restarts_positions():
    ref = stream_ref.StreamRef(C, 0.01, 1, 4, 1 << 20)
    x = np.zeros(3 * C + 10, dtype=np.int16)
    x[3 * C:] = 9000                                        # only the 10-sample partial chunk is loud
    assert ref.push(x[:100]) == [] and ref.push(x[100:]) == []
    assert ref.push(x[:0], close=True) == [(3 * C, 3 * C + 10, stream_ref.FLUSHED)]
    assert (ref.n, ref.j, ref.recording) == (0, 0, False)
    y = np.full(2 * C, 9000, dtype=np.int16)
    assert ref.push(np.concatenate([y, np.zeros(4 * C, np.int16)])) == [(0, 6 * C, 0)]


def test_size_helpers():
    lib = _native.lib()
    byref = ctypes.byref
    assert lib.sir_stream_min_ring_chunks(byref(_cfg())) == 12 + 4 + 2          # M + ceil(200 / 64) + 2
    assert lib.sir_stream_max_rows(byref(_cfg())) == 4 * (4 + 2)
    assert lib.sir_stream_min_ring_chunks(byref(_cfg(c=1024, max_in=1024, prior=7, n_stop=16, M=157))) == 157 + 1 + 2
    assert lib.sir_stream_max_rows(byref(_cfg(c=1024, max_in=1024, prior=7, S=1024, M=157))) == 3 * 1024
    assert lib.sir_stream_max_rows(byref(_cfg(max_in=1))) == 4 * 3
    assert lib.sir_stream_max_rows(byref(_cfg(max_in=64))) == 4 * 3 and lib.sir_stream_max_rows(byref(_cfg(max_in=65))) == 4 * 4
    # neither helper looks at ring_chunks; every other field is checked
    assert lib.sir_stream_min_ring_chunks(byref(_cfg(R=0))) == 18
    for bad in (_cfg(c=100), _cfg(thr=float("nan")), _cfg(n_stop=-1), _cfg(prior=-1), _cfg(S=0), _cfg(S=65536), _cfg(dtype=5),
                _cfg(max_in=0), _cfg(M=3), _cfg(M=2)):
        assert lib.sir_stream_min_ring_chunks(byref(bad)) == -1
        assert lib.sir_stream_max_rows(byref(bad)) == -1
        assert lib.sir_stream_state_bytes(None, byref(bad)) == 0
    assert lib.sir_stream_min_ring_chunks(None) == -1 and lib.sir_stream_max_rows(None) == -1
    # the calls themselves refuse a NULL handle before they look at anything else
    assert lib.sir_stream_push(None, None, 0, byref(_cfg()), None, 0, 0, None, None, None, None, 0, None, None) == _native.SIR_EINVAL
    assert lib.sir_stream_reset(None, None, 0, byref(_cfg()), None, None) == _native.SIR_EINVAL
    assert lib.sir_stream_gather(None, None, 0, byref(_cfg()), None, None, 0, None, 0, 0, None, None) == _native.SIR_EINVAL


def test_stream_segmenter_arguments():
    s = StreamSegmenter(1024, 1024)
    assert (s.sample_rate, s.chunk_size, s.prior_chunks, s.silence_chunks, s.flush_tail) == (16000, 1024, 7, 16, True)
    assert s.max_utt_chunks == 157 and s.chunks_per_push == 1 and s.ring_chunks == s.min_ring_chunks == 160       # ceil(10 s / 64 ms)
    assert s.max_rows == 3 * 1024 and s.dtype == torch.int16
    cfg = s.config()
    assert (cfg.vad.chunk_size, cfg.vad.silence_chunks, cfg.vad.prior_chunks, cfg.vad.flush_tail) == (1024, 16, 7, 1)
    assert (cfg.n_streams, cfg.wave_dtype, cfg.max_in, cfg.max_utt_chunks, cfg.ring_chunks) == (1024, _native.WAVE_I16, 1024, 157, 160)
    lib = _native.lib()
    assert lib.sir_stream_min_ring_chunks(ctypes.byref(cfg)) == s.min_ring_chunks
    assert lib.sir_stream_max_rows(ctypes.byref(cfg)) == s.max_rows
    s = StreamSegmenter(5, 200, dtype=torch.float32, chunk_size=64, silence_limit=2 * 64 / 16000, prior_recording=3.5 * 64 / 16000,
                        max_utt_chunks=12)
    assert (s.prior_chunks, s.silence_chunks, s.ring_chunks, s.max_rows) == (3, 2, 18, 30)
    for bad in (dict(n_streams=0), dict(n_streams=65536), dict(n_streams=2.5), dict(max_push=0), dict(dtype=torch.float64),
                dict(max_utterance=0), dict(max_utterance=float("inf")), dict(max_utterance=0.4),     # 7 chunks: not above the prior 7
                dict(max_utt_chunks=7), dict(ring_chunks=159), dict(chunk_size=100), dict(threshold=-0.1), dict(silence_limit=-1)):
        args = dict(n_streams=4, max_push=1024)
        args.update(bad)
        with pytest.raises(ValueError):
            StreamSegmenter(**args)


def test_stream_segmenter_refuses_to_run_without_a_gpu():
    if torch.cuda.is_available():
        samples = torch.zeros((2, 64), dtype=torch.float64, device="cuda")
    else:
        samples = torch.zeros((2, 64), dtype=torch.int16)
    with pytest.raises(_native.SirError):
        StreamSegmenter(2, 64).push(samples)
