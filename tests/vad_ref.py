"""Host reference of the utterance segmenter (``sir_vad_segment`` / ``sir_vad_gather``), plain numpy.

``segments_loop`` is the listener's state machine run chunk by chunk over a vector of speech flags, the way
``MicrophoneListener.listen`` runs it over a stream, with the two documented differences of include/sir_hip.h: the trigger chunk
appears once in a segment, and ``flush_tail`` emits an utterance still open at the end.  ``segments_parallel`` is the same
function written the way the kernel computes it (prefix maximum of the last speech chunk, prefix sums of the trigger and end
flags); tests/test_vad_host.py holds the two against each other.  Energies are formed in float64.
"""
import numpy as np


def n_chunks(length, c):
    return (int(length) + c - 1) // c


def chunk_energy(x, length, c):
    """float64 mean |x| of every chunk of x[:length] (int16 is dequantised as s / 32768); a trailing partial chunk is judged on
    its own samples"""
    x = np.asarray(x)[:int(length)]
    scale = 32768.0 if x.dtype == np.int16 else 1.0
    n = n_chunks(length, c)
    a = np.zeros(n * c, dtype=np.float64)
    a[:len(x)] = np.abs(x.astype(np.float64))
    count = np.full(n, c, dtype=np.float64)
    if n:
        count[-1] = len(x) - (n - 1) * c
    return a.reshape(n, c).sum(axis=1) / (count * scale)


def speech_flags(x, length, c, threshold):
    """the listener's decision: float32 energy strictly above the float32 threshold"""
    return chunk_energy(x, length, c).astype(np.float32) > np.float32(threshold)


def segments_loop(flags, length, c, prior_chunks, silence_chunks, flush_tail=True):
    """-> list of (start sample, end sample), in time order"""
    segs = []
    recording = False
    silence = 0
    first = 0
    for i, speech in enumerate(flags):
        if not recording and speech:
            recording = True
            silence = 0
            first = max(0, i - prior_chunks + 1) if prior_chunks >= 1 else i
        if recording:
            silence = 0 if speech else silence + 1
            if silence >= silence_chunks:
                segs.append((first * c, min((i + 1) * c, int(length))))
                recording = False
    if recording and flush_tail:
        segs.append((first * c, int(length)))
    return segs


def segments_parallel(flags, length, c, prior_chunks, silence_chunks, flush_tail=True):
    """the same function without a loop-carried state: every chunk decides from the prefix maximum ``last``"""
    f = np.asarray(flags, dtype=bool)
    n = len(f)
    if n == 0:
        return []
    idx = np.arange(n)
    last_upto = np.maximum.accumulate(np.where(f, idx, -1))            # latest speech chunk <= i, -1 = none
    last_before = np.concatenate(([-1], last_upto[:-1]))
    trigger = f & ((last_before < 0) | (idx - last_before > silence_chunks))
    end = (last_upto >= 0) & (idx - last_upto == silence_chunks)
    ti, ej = idx[trigger], idx[end]
    first = np.maximum(0, ti - prior_chunks + 1) if prior_chunks >= 1 else ti
    starts = first * c
    ends = np.minimum((ej + 1) * c, int(length))
    assert len(ti) - len(ej) in (0, 1)
    if len(ti) > len(ej):                                               # open at the end of the recording
        assert last_upto[-1] + silence_chunks >= n
        if flush_tail:
            ends = np.concatenate((ends, [int(length)]))
        else:
            starts = starts[:-1]
    return [(int(s), int(e)) for s, e in zip(starts, ends)]


def segment_batch(waves, lengths, c, threshold, prior_chunks, silence_chunks, flush_tail=True, flags=None):
    """-> (seg_count int32 [n_rec], table int32 [total, 3] = {recording, start, end}, recording-major then by time)"""
    counts, rows = [], []
    for r, length in enumerate(lengths):
        fl = flags[r] if flags is not None else speech_flags(waves[r], length, c, threshold)
        segs = segments_loop(fl, length, c, prior_chunks, silence_chunks, flush_tail)
        counts.append(len(segs))
        rows += [(r, s, e) for s, e in segs]
    return np.asarray(counts, dtype=np.int32), np.asarray(rows, dtype=np.int32).reshape(-1, 3)


def gather(waves, table, max_clip_len):
    """-> (clips float32 [n, max_clip_len] zero behind each length, lengths int32 [n])"""
    out = np.zeros((len(table), max_clip_len), dtype=np.float32)
    lens = np.zeros(len(table), dtype=np.int32)
    for s, (r, a, b) in enumerate(table):
        x = np.asarray(waves[r])[a:b][:max_clip_len]
        if x.dtype == np.int16:
            x = x.astype(np.float32) / np.float32(32768.0)
        out[s, :len(x)] = x
        lens[s] = len(x)
    return out, lens
