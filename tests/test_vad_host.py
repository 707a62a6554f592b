"""CPU: the segmenter's reference (tests/vad_ref.py) on hand-worked cases, its data-parallel form against its sequential loop,
the host helper ``sir_vad_stop_chunks`` and ``Segmenter``'s argument handling.  No GPU."""
import numpy as np
import pytest

import vad_ref
from sir_amd import _native
from sir_amd.segmenter import Segmenter

C = 64


def _flags(n, speech):
    f = np.zeros(n, dtype=bool)
    f[list(speech)] = True
    return f


def _both(flags, length, P, n_stop, flush=True):
    a = vad_ref.segments_loop(flags, length, C, P, n_stop, flush)
    b = vad_ref.segments_parallel(flags, length, C, P, n_stop, flush)
    assert a == b
    return a


def test_single_burst():
    # speech at chunks 5..7, n_stop 3: the silence run reaches 3 at chunk 10; prior 2 -> first chunk 5 - 2 + 1 = 4
    f = _flags(20, [5, 6, 7])
    assert _both(f, 20 * C, 2, 3) == [(4 * C, 11 * C)]


def test_two_bursts_n_stop_apart_are_one_segment():
    # speech at 2 and at 2 + 3: the run behind chunk 2 is only 2 long when chunk 5 speaks
    f = _flags(20, [2, 5])
    assert _both(f, 20 * C, 1, 3) == [(2 * C, 9 * C)]


def test_two_bursts_n_stop_plus_one_apart_overlap_by_the_prior_buffer():
    # speech at 2 and 6, n_stop 3: the first segment ends at chunk 5, the second triggers at 6 and, with a prior buffer of 3
    # chunks that is not cleared between utterances, starts at chunk 4 -- inside the first
    f = _flags(20, [2, 6])
    assert _both(f, 20 * C, 3, 3) == [(0, 6 * C), (4 * C, 10 * C)]


def test_burst_at_chunk_zero_with_prior_larger_than_the_index():
    f = _flags(10, [0, 1])
    assert _both(f, 10 * C, 7, 2) == [(0, 4 * C)]


def test_no_prior_buffer():
    f = _flags(10, [3])
    assert _both(f, 10 * C, 0, 2) == [(3 * C, 6 * C)]
    assert _both(f, 10 * C, 1, 2) == [(3 * C, 6 * C)]          # a buffer of one chunk holds the trigger chunk only


def test_n_stop_zero_makes_every_speech_chunk_a_segment():
    f = _flags(8, [1, 2, 5])
    assert _both(f, 8 * C, 0, 0) == [(1 * C, 2 * C), (2 * C, 3 * C), (5 * C, 6 * C)]
    assert _both(f, 8 * C, 2, 0) == [(0, 2 * C), (1 * C, 3 * C), (4 * C, 6 * C)]


def test_open_tail_flush_on_and_off():
    # speech at chunk 7 of 9 chunks (the last one 10 samples long), n_stop 4: still open when the recording stops
    f = _flags(9, [1, 7])
    length = 8 * C + 10
    assert _both(f, length, 1, 4, flush=True) == [(1 * C, 6 * C), (7 * C, length)]
    assert _both(f, length, 1, 4, flush=False) == [(1 * C, 6 * C)]
    # the run reaches n_stop exactly on the last chunk: closed by the state machine itself, with or without the flush
    f = _flags(9, [4])
    assert _both(f, length, 1, 4, flush=False) == [(4 * C, length)]


def test_all_silent_and_empty():
    assert _both(_flags(12, []), 12 * C, 7, 16) == []
    assert _both(_flags(0, []), 0, 7, 16) == []
    counts, table = vad_ref.segment_batch([np.zeros(0, np.int16), np.zeros(100, np.int16)], [0, 100], C, 0.01, 7, 16)
    assert counts.tolist() == [0, 0] and table.shape == (0, 3)


def test_energy_and_partial_chunk():
    x = np.zeros(C + 3, dtype=np.int16)
    x[:C] = 256
    x[C:] = [-32768, 0, 32767]
    e = vad_ref.chunk_energy(x, len(x), C)
    assert e[0] == 256 / 32768 and e[1] == (32768 + 32767) / (3 * 32768.0)
    assert vad_ref.speech_flags(x, len(x), C, 2.0 ** -7).tolist() == [False, True]      # strict: 2^-7 is not above 2^-7
    clips, lens = vad_ref.gather([x], np.array([[0, 0, C + 3]], dtype=np.int32), C + 1)
    assert lens.tolist() == [C + 1] and clips[0, C] == -1.0 and clips[0, 0] == np.float32(256 / 32768)


def test_parallel_form_equals_the_loop_on_random_flags():
    """12 000 random flag vectors: lengths 1-60, P 0-4, n_stop 0-4, four speech densities, both flush settings, the last chunk
    partial or whole"""
    rng = np.random.default_rng(20240607)
    n_cases = 0
    for density in (0.05, 0.2, 0.5, 0.9):
        for _ in range(3000):
            n = int(rng.integers(1, 61))
            f = rng.random(n) < density
            P, n_stop = int(rng.integers(0, 5)), int(rng.integers(0, 5))
            length = n * C - int(rng.integers(0, C))
            flush = bool(rng.integers(0, 2))
            a = vad_ref.segments_loop(f, length, C, P, n_stop, flush)
            b = vad_ref.segments_parallel(f, length, C, P, n_stop, flush)
            assert a == b, (f.astype(int).tolist(), length, P, n_stop, flush)
            n_cases += 1
    assert n_cases >= 10000


def test_stop_chunks_helper():
    lib = _native.lib()
    assert lib.sir_vad_stop_chunks(16000, 1024, 1.0) == 16          # 15 * 0.064 = 0.96 < 1 <= 16 * 0.064
    assert lib.sir_vad_stop_chunks(16000, 1024, 0.0) == 0
    assert lib.sir_vad_stop_chunks(16000, 64, 1.0) == 250           # 250 * 0.004 == 1.0 in double
    for sr, c, lim in ((16000, 1024, 1.0), (8000, 512, 0.3), (44100, 4096, 2.5), (16000, 64, 0.5), (22050, 320, 1.0)):
        n = lib.sir_vad_stop_chunks(sr, c, lim)
        want = next(k for k in range(100000) if k * (c / sr) >= lim)        # the listener's own expression
        assert n == want
    assert lib.sir_vad_stop_chunks(0, 1024, 1.0) == -1
    assert lib.sir_vad_stop_chunks(16000, 0, 1.0) == -1
    assert lib.sir_vad_stop_chunks(16000, 1024, -1.0) == -1
    assert lib.sir_vad_stop_chunks(16000, 1024, float("nan")) == -1
    assert lib.sir_vad_stop_chunks(16000, 1024, float("inf")) == -1


def test_segmenter_arguments():
    s = Segmenter()
    assert (s.sample_rate, s.chunk_size, s.prior_chunks, s.silence_chunks, s.flush_tail) == (16000, 1024, 7, 16, True)
    assert s.threshold == 0.01
    cfg = s.config()
    assert (cfg.chunk_size, cfg.silence_chunks, cfg.prior_chunks, cfg.flush_tail) == (1024, 16, 7, 1)
    assert cfg.threshold == np.float32(0.01)
    s = Segmenter(sample_rate=8000, chunk_size=64, threshold=0, silence_limit=0, prior_recording=0, flush_tail=False)
    assert (s.prior_chunks, s.silence_chunks, s.config().flush_tail) == (0, 0, 0)
    for bad in (dict(chunk_size=100), dict(chunk_size=32), dict(chunk_size=8192), dict(threshold=float("nan")), dict(threshold=-0.1),
                dict(silence_limit=-1), dict(silence_limit=float("inf")), dict(prior_recording=-0.5), dict(sample_rate=0)):
        with pytest.raises(ValueError):
            Segmenter(**bad)


def test_segmenter_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        wave = torch.zeros((1, 128), dtype=torch.float64, device="cuda")
    else:
        wave = torch.zeros((1, 128), dtype=torch.int16)
    with pytest.raises(_native.SirError):
        Segmenter().segment(wave)
