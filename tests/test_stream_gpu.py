"""GPU: live streams (sir_stream_push / sir_stream_gather, sir_amd.streaming, IntentRecognizer.open_streams) against the shipped
batch form (sir_amd.segmenter.Segmenter on the whole recordings) and the numpy references tests/vad_ref.py / tests/stream_ref.py.

Inputs.  Chunks of 64 samples unless stated.  A recording is silence (exact zeros) with bursts of noise, |x| in [0.1, 0.2] with a
random sign, 1-6 chunks long, that start and stop off the chunk grid but cover at least a quarter of every chunk they touch: a
chunk's energy is 0 or >= 0.1 / 4 = 2.5 x the threshold 0.01 (asserted on the reference energies), so no decision hinges on a
rounding and the float32 tables can be compared exactly.  Clips are copies (int16: one exact scaling), compared bit for bit.

Seams covered: pushes smaller than a chunk (63, and 1 sample), pushes of several chunks (200, 1000), a chunk assembled from three
pushes, destination offsets of every alignment, the ring wrap (R at its minimum), several rows of one stream in one push, an
utterance over several pushes, the forced cut with overlapping rows, close + slot reuse, streams that get nothing in a push.

Measured on MI355X: every comparison here is exact and holds, the logits of the end-to-end test included; the whole file runs in
about 2 s, its slowest case (end to end, 111 feeds) in under 1 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import stream_ref
import vad_ref
from sir_amd import _native, ops, synth
from sir_amd.models.models import CNNAudioGRU
from sir_amd.segmenter import Segmenter
from sir_amd.streaming import StreamSegmenter

pytestmark = pytest.mark.gpu
DEV = "cuda"
CH = 64
THR = 0.01
SR = 16000
LENGTHS = [0, 63, 1000, 4037, 4992]
HUGE = 1 << 12                                   # max_utt_chunks no utterance here can reach (the longest recording has 78 chunks)
WRAP_SEED = 1                                    # test_segments_across_the_ring_wrap: a seed whose recording has such segments
TORCH_DT = {np.dtype(np.int16): torch.int16, np.dtype(np.float32): torch.float32}


def _bursty(rng, length, dtype, c=CH, burst=(1, 6), gap=(3, 8), loud_all=False):
    """silence with noise bursts; a burst begins and ends 16 .. 48 samples into a chunk"""
    x = np.zeros(length, dtype=np.float64)
    mag = rng.uniform(0.1, 0.2, length) * (rng.integers(0, 2, length) * 2 - 1)
    if loud_all:
        x[:] = mag
    else:
        k = int(rng.integers(0, gap[1]))
        while k * c < length:
            n = int(rng.integers(burst[0], burst[1] + 1))
            a = k * c + int(rng.integers(16, 49))
            b = (k + n - 1) * c + int(rng.integers(16, 49)) if n > 1 else k * c + c
            b = max(b, a + 16) if n > 1 else b
            x[a:min(b, length)] = mag[a:min(b, length)]
            k += n + int(rng.integers(gap[0], gap[1] + 1))
    if np.dtype(dtype) == np.int16:
        return np.round(x * 32767.0).astype(np.int16)
    return x.astype(np.float32)


def _check_margin(recs, c=CH):
    for x in recs:
        e = vad_ref.chunk_energy(x, len(x), c)
        assert ((e <= THR / 2) | (e >= 2 * THR)).all()


def _listener(c, P, n_stop):
    """listener arguments that give prior_chunks P and silence_chunks n_stop at 16 kHz"""
    return dict(sample_rate=SR, chunk_size=c, threshold=THR, silence_limit=max(0.0, (n_stop - 0.5) * c / SR),
                prior_recording=(P + 0.5) * c / SR)


def _segmenters(S, max_push, dtype, P, n_stop, M=HUGE, ring=None, c=CH):
    seg = Segmenter(flush_tail=True, **_listener(c, P, n_stop))
    ss = StreamSegmenter(S, max_push, dtype=TORCH_DT[np.dtype(dtype)], device=DEV, max_utt_chunks=M, ring_chunks=ring, flush_tail=True,
                         **_listener(c, P, n_stop))
    assert (seg.prior_chunks, seg.silence_chunks) == (ss.prior_chunks, ss.silence_chunks) == (P, n_stop)
    return seg, ss


def _plan(recs, pieces):
    """per stream the list of (samples, close) it hands over push by push: recording s cut as pieces[s], closed with its last piece"""
    plan = []
    for x, p in zip(recs, pieces):
        assert sum(p) == len(x)
        at, ev = 0, []
        for k, m in enumerate(p):
            ev.append((x[at:at + m], k == len(p) - 1))
            at += m
        plan.append(ev if ev else [(x[:0], True)])
    return plan


def _feed(ss, plan, max_clip, dtype):
    """run a plan -> (rows per stream [(start, end, flags)], clips per stream, the raw (table, clips, lengths) of every push)"""
    S = ss.n_streams
    rows, clips, raw = [[] for _ in range(S)], [[] for _ in range(S)], []
    for k in range(max(len(ev) for ev in plan)):
        now = [ev[k] if k < len(ev) else (None, False) for ev in plan]
        width = max([1] + [len(x) for x, _ in now if x is not None])
        host = np.zeros((S, width), dtype=dtype)
        lens = np.zeros(S, dtype=np.int32)
        for s, (x, _) in enumerate(now):
            if x is not None:
                host[s, :len(x)] = x
                lens[s] = len(x)
        close = [s for s, (_, cl) in enumerate(now) if cl]
        out, out_len, table = ss.push(torch.from_numpy(host).to(DEV), torch.from_numpy(lens).to(DEV), close=close, max_clip_len=max_clip)
        t, o, n = table.cpu().numpy(), out.cpu().numpy(), out_len.cpu().numpy()
        raw.append((t, o, n))
        assert t.dtype == np.int64 and t.shape[1:] == (4,) and o.shape == (len(t), max_clip)
        key = [(int(r[0]), int(r[2])) for r in t]                   # stream-major, then by time (ends of one stream ascend)
        assert key == sorted(key)
        for r, row in enumerate(t):
            assert n[r] == min(row[2] - row[1], max_clip) and not o[r, n[r]:].any()
            rows[row[0]].append((int(row[1]), int(row[2]), int(row[3])))
            clips[row[0]].append(o[r, :n[r]])
    return rows, clips, raw


def _batch(seg, recs, dtype, max_clip):
    """the shipped batch form on the whole recordings -> (table [n, 3], clips [n, max_clip], lengths), host arrays"""
    width = -(-max(max(len(x) for x in recs), 8) // 8) * 8
    wave = np.zeros((len(recs), width), dtype=dtype)
    for r, x in enumerate(recs):
        wave[r, :len(x)] = x
    dw = torch.from_numpy(wave).to(DEV)
    dl = torch.tensor([len(x) for x in recs], dtype=torch.int32, device=DEV)
    table, _, total = seg.segment(dw, dl)
    out, out_len = seg.gather(dw, table, total, max_clip)
    return table.cpu().numpy(), out.cpu().numpy(), out_len.cpu().numpy()


def _assert_equals_batch(rows, clips, seg, recs, dtype, max_clip, P, n_stop, c=CH):
    """streamed rows / clips == the batch form's == vad_ref's, stream by stream"""
    table, out, out_len = _batch(seg, recs, dtype, max_clip)
    _, ref = vad_ref.segment_batch(recs, [len(x) for x in recs], c, THR, P, n_stop, True)
    assert np.array_equal(table, ref)
    want, want_len = vad_ref.gather(recs, ref, max_clip)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32)) and np.array_equal(out_len, want_len)
    got = [(s, a, b) for s in range(len(recs)) for a, b, _ in rows[s]]
    assert got == [tuple(r) for r in ref.tolist()]
    flat = [cl for s in range(len(recs)) for cl in clips[s]]
    for r, cl in enumerate(flat):
        assert np.array_equal(cl.view(np.uint32), out[r, :out_len[r]].view(np.uint32)), r
    for s, x in enumerate(recs):                                   # flags: only a row that ends with the recording can be the flush
        for a, b, fl in rows[s]:
            assert fl in (0, stream_ref.FLUSHED) and (fl == 0 or b == len(x))


def _random_pieces(rng, total, most):
    out = []
    while total > 0:
        m = min(total, int(rng.integers(0, most + 1)))
        out.append(m)
        total -= m
    return out


_recs = {}


def _recordings(dtype):
    key = np.dtype(dtype).name
    if key not in _recs:
        rng = np.random.default_rng(7)
        _recs[key] = [_bursty(rng, n, dtype) for n in LENGTHS]
        _check_margin(_recs[key])
    return _recs[key]


# ---- 1. chunking invariance against the shipped batch form -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["i16", "f32"])
@pytest.mark.parametrize("schedule", ["fixed1000", "rand63", "rand200", "rand1000"])
def test_any_cut_into_pushes_gives_the_batch_form(schedule, dtype):
    recs = _recordings(dtype)
    max_in = 1000 if schedule == "fixed1000" else int(schedule[4:])
    rng = np.random.default_rng(11 + max_in)
    n_rows = 0
    for P in (0, 1, 3):
        for n_stop in (0, 2):
            seg, ss = _segmenters(len(recs), max_in, dtype, P, n_stop)
            if schedule == "fixed1000":
                pieces = [[1000] * (len(x) // 1000) + ([len(x) % 1000] if len(x) % 1000 else []) for x in recs]
            else:
                pieces = [_random_pieces(rng, len(x), max_in) for x in recs]
            rows, clips, _ = _feed(ss, _plan(recs, pieces), 1200, dtype)
            _assert_equals_batch(rows, clips, seg, recs, dtype, 1200, P, n_stop)
            n_rows += sum(len(r) for r in rows)
    assert n_rows > 60
    ops.check_status()


@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["i16", "f32"])
def test_one_sample_per_push(dtype):
    rng = np.random.default_rng(5)
    recs = [_bursty(rng, 640, dtype, gap=(2, 3), burst=(1, 2))]
    _check_margin(recs)
    seg, ss = _segmenters(1, 1, dtype, 1, 2)
    rows, clips, _ = _feed(ss, _plan(recs, [[1] * 640]), 640, dtype)
    assert len(rows[0]) >= 2
    _assert_equals_batch(rows, clips, seg, recs, dtype, 640, 1, 2)
    ops.check_status()


# ---- 2. same energies ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["i16", "f32"])
def test_energy_of_a_chunk_assembled_from_three_pushes_equals_the_batch_form(dtype):
    """stream 0 cuts every chunk 23 + 22 + 19, stream 1 takes 50 + 40 + 38 (chunks from two or three pushes, unaligned ring
    offsets), stream 2 whole chunks; the trailing 37-sample chunk is judged at the close.  Bit-equal to sir_vad_segment's energy_out."""
    rng = np.random.default_rng(21)
    length = 10 * CH + 37
    recs = [_bursty(rng, length, dtype, gap=(1, 2), burst=(1, 3)) for _ in range(3)]
    cycles = [(23, 22, 19), (50, 40, 38), (64, 64, 64)]
    pieces = []
    for cyc in cycles:
        p, left, k = [], length, 0
        while left > 0:
            p.append(min(left, cyc[k % 3]))
            left -= p[-1]
            k += 1
        pieces.append(p)
    seg, ss = _segmenters(3, 64, dtype, 1, 2)
    plan = _plan(recs, pieces)
    got = [[] for _ in recs]
    n = [0, 0, 0]
    for k in range(max(len(ev) for ev in plan)):
        host = np.zeros((3, 64), dtype=dtype)
        lens = np.zeros(3, dtype=np.int32)
        close = []
        judged = []
        for s, ev in enumerate(plan):
            x, cl = ev[k] if k < len(ev) else (recs[s][:0], False)
            host[s, :len(x)] = x
            lens[s] = len(x)
            before = n[s] // CH
            n[s] += len(x)
            judged.append(n[s] // CH - before + (1 if cl and n[s] % CH else 0))
            if cl:
                close.append(s)
                n[s] = 0
        e = torch.full((3, ss.chunks_per_push + 1), -1.0, dtype=torch.float32, device=DEV)
        ss.push_table(torch.from_numpy(host).to(DEV), torch.from_numpy(lens).to(DEV), close=close, energy_out=e)
        e = e.cpu().numpy()
        for s in range(3):
            got[s] += e[s, :judged[s]].tolist()
            assert not e[s, judged[s]:].any()                       # zero behind the chunks this push judged
    wave = np.zeros((3, 11 * CH), dtype=dtype)
    for r, x in enumerate(recs):
        wave[r, :length] = x
    want = torch.full((3, 11), -1.0, dtype=torch.float32, device=DEV)
    seg.segment(torch.from_numpy(wave).to(DEV), torch.full((3,), length, dtype=torch.int32, device=DEV), energy_out=want)
    want = want.cpu().numpy()
    assert (want > 2 * THR).any() and (want == 0).any()
    for s in range(3):
        assert np.array_equal(np.asarray(got[s], dtype=np.float32).view(np.uint32), want[s].view(np.uint32)), s
    ops.check_status()


# ---- 3. ring wrap ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["i16", "f32"])
def test_segments_across_the_ring_wrap(dtype):
    """R at its minimum 12 + 4 + 2 = 18 chunks = 1152 samples, a 5037-sample stream (4.4 ring lengths) in pushes of 0 .. 200;
    bursts of 1-5 chunks + P 3 + n_stop 2 stay below M = 12, so nothing is forced and the batch form is the reference"""
    P, n_stop, M, R = 3, 2, 12, 18
    rng = np.random.default_rng(WRAP_SEED)
    recs = [_bursty(rng, 5037, dtype, burst=(1, 5), gap=(3, 8))]
    _check_margin(recs)
    _, ref = vad_ref.segment_batch(recs, [5037], CH, THR, P, n_stop, True)
    laps = [(a // (R * CH), (b - 1) // (R * CH)) for _, a, b in ref.tolist()]
    assert sum(1 for la, lb in laps if la != lb) >= 1 and max(b - a for _, a, b in ref.tolist()) < M * CH
    seg, ss = _segmenters(1, 200, dtype, P, n_stop, M=M, ring=R)
    assert ss.min_ring_chunks == R
    rows, clips, _ = _feed(ss, _plan(recs, [_random_pieces(rng, 5037, 200)]), M * CH, dtype)
    _assert_equals_batch(rows, clips, seg, recs, dtype, M * CH, P, n_stop)
    ops.check_status()
    # hand-written rows over the R * CH samples the ring still holds (a close moves the counters, not the ring; the detector
    # only ever starts a clip on a chunk boundary), around position `wrap`, which sits at ring offset 0: an aligned start whose
    # 16-byte groups meet the wrap, a start off the 16-byte grid with the wrap inside the clip, both cut at max_clip_len, an
    # aligned start whose clip ends inside a group, a one-sample clip; then a stream outside the slots (a zero row, reported)
    # and a row at the total (length 0 only).  204 columns: aligned output rows; 203: rows no vector store may touch.
    x, wrap = recs[0], len(recs[0]) // (R * CH) * (R * CH)
    assert len(x) - R * CH < wrap - 300 and wrap + 300 < len(x)
    hand = [(wrap - 128, wrap + 128, 0), (wrap - 107, wrap + 193, 0), (wrap + 64, wrap + 101, 0), (wrap - 298, wrap - 297, 0)]
    n = len(hand)
    table = torch.tensor([[0, a, b, f] for a, b, f in hand] + [[1, wrap, wrap + 64, 0], [0, wrap, wrap + 64, 0]], dtype=torch.int64, device=DEV)
    total = torch.tensor([n + 1], dtype=torch.int32, device=DEV)
    for max_clip in (204, 203):
        out, out_len = ss.gather(table, total, max_clip)
        got, got_len = out.cpu().numpy(), out_len.cpu().numpy()
        want, want_len = stream_ref.gather(x, hand, max_clip)
        assert want_len.tolist() == [max_clip, max_clip, 37, 1]
        assert np.array_equal(got[:n].view(np.uint32), want.view(np.uint32)) and np.array_equal(got_len[:n], want_len)
        assert not got[n].any() and got_len[n:].tolist() == [0, 0]
        with pytest.raises(_native.SirError, match="sir_stream_gather"):
            ops.check_status()
    ops.check_status()



# ---- 4. several utterances of one stream in one push; one utterance over several pushes ----------------------------------------
def test_four_rows_of_one_stream_in_one_push_and_an_utterance_over_three_pushes():
    rng = np.random.default_rng(31)
    loud = lambda n: (rng.uniform(0.1, 0.2, n) * (rng.integers(0, 2, n) * 2 - 1)).astype(np.float32)
    a = np.zeros(1000, dtype=np.float32)
    for k in (1, 4, 7, 10):
        a[k * CH + 20:(k + 1) * CH] = loud(CH - 20)
    b = np.zeros(3000, dtype=np.float32)
    b[150:2600] = loud(2450)
    recs = [a, b]
    _check_margin(recs)
    seg, ss = _segmenters(2, 1000, np.float32, 1, 1)
    rows, clips, raw = _feed(ss, _plan(recs, [[1000], [1000, 1000, 1000]]), 3000, np.float32)
    assert [r[:2] for r in rows[0]] == [(k * CH, (k + 2) * CH) for k in (1, 4, 7, 10)]
    assert (raw[0][0][:, 0] == 0).sum() == 4                        # all four came out of the first push
    assert rows[1] == [(2 * CH, 42 * CH, 0)] and len(raw[0][0]) == 4 and len(raw[1][0]) == 0 and len(raw[2][0]) == 1
    _assert_equals_batch(rows, clips, seg, recs, np.float32, 3000, 1, 1)
    ops.check_status()


# ---- 5. forced cut ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["i16", "f32"])
def test_forced_cut_rows_and_their_overlapping_clips(dtype):
    P, n_stop, M = 3, 2, 12
    rng = np.random.default_rng(41)
    x = _bursty(rng, 40 * CH, dtype, loud_all=True)
    F, L = stream_ref.FORCED, stream_ref.FLUSHED
    want = [(0, 768, F), (640, 1408, F), (1280, 2048, F), (1920, 2560, L)]
    pieces = _random_pieces(rng, len(x), 200)
    assert stream_ref.run(x, pieces, CH, THR, P, n_stop, M) == want
    _, ss = _segmenters(1, 200, dtype, P, n_stop, M=M, ring=18)
    rows, clips, _ = _feed(ss, _plan([x], [pieces]), M * CH, dtype)
    assert rows[0] == want
    ref_clips, ref_len = stream_ref.gather(x, want, M * CH)
    for r, cl in enumerate(clips[0]):
        assert np.array_equal(cl.view(np.uint32), ref_clips[r, :ref_len[r]].view(np.uint32)), r
    assert np.array_equal(clips[0][0][640:], clips[0][1][:128])    # the overlap of consecutive rows holds the same samples
    ops.check_status()


# ---- 6. close and slot reuse -----------------------------------------------------------------------------------------------
def test_close_halfway_and_reuse_of_the_slot():
    P, n_stop = 1, 2
    rng = np.random.default_rng(51)
    recs = [_bursty(rng, 2000, np.int16) for _ in range(2)]
    # caller a ends 37 samples into chunk 16 with |s| = 500: mean 500 / 32768 = 0.0153 over its own samples is speech, over a whole
    # chunk (0.0088) it would not be.  int16 energies are exact, so this decision does not hinge on a rounding either.
    caller_a = np.zeros(16 * CH + 37, dtype=np.int16)
    caller_a[5 * CH + 20:7 * CH] = 5000
    caller_a[16 * CH:] = -500
    caller_b = _bursty(rng, 1500, np.int16)
    _check_margin(recs + [caller_b])
    cut = lambda x: [200] * (len(x) // 200) + ([len(x) % 200] if len(x) % 200 else [])
    # slot 2: caller a, closed with its last samples, then caller b in the same slot
    ev2 = _plan([caller_a], [cut(caller_a)])[0] + _plan([caller_b], [cut(caller_b)])[0]
    plan = _plan(recs[:2], [cut(recs[0]), cut(recs[1])]) + [ev2]
    _, ss = _segmenters(3, 200, np.int16, P, n_stop)
    rows, clips, _ = _feed(ss, plan, 2000, np.int16)
    want_a = stream_ref.run(caller_a, cut(caller_a), CH, THR, P, n_stop, HUGE)
    want_b = stream_ref.run(caller_b, cut(caller_b), CH, THR, P, n_stop, HUGE)
    assert want_a == [(5 * CH, 9 * CH, 0), (16 * CH, len(caller_a), stream_ref.FLUSHED)]
    assert want_b and want_b[0][0] < want_a[-1][0]                  # b's positions restart at 0
    assert rows[2] == want_a + want_b
    both = np.concatenate([caller_a, caller_b])
    ref_clips, ref_len = vad_ref.gather([caller_a] * len(want_a) + [caller_b] * len(want_b),
                                        [(r, a, b) for r, (a, b, _) in enumerate(want_a + want_b)], 2000)
    for r, cl in enumerate(clips[2]):
        assert np.array_equal(cl.view(np.uint32), ref_clips[r, :ref_len[r]].view(np.uint32)), r
    # the other streams: as in a run in which slot 2 is never closed halfway
    _, ss2 = _segmenters(3, 200, np.int16, P, n_stop)
    rows2, clips2, _ = _feed(ss2, _plan(recs[:2] + [both], [cut(recs[0]), cut(recs[1]), cut(both)]), 2000, np.int16)
    for s in (0, 1):
        assert rows[s] == rows2[s] and len(rows[s]) >= 2
        assert all(np.array_equal(p, q) for p, q in zip(clips[s], clips2[s]))
    # reset() forgets an open utterance without emitting it
    ss.push(torch.full((3, 200), 6000, dtype=torch.int16, device=DEV))
    ss.reset([1])
    out, out_len, table = ss.push(torch.zeros((3, 1), dtype=torch.int16, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV),
                                  close=[0, 1, 2])
    assert table.cpu().numpy().tolist() == [[0, 0, 200, 2], [2, 0, 200, 2]]
    ops.check_status()


# ---- 7. order and determinism ----------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes():
    recs = _recordings(np.float32)
    rng = np.random.default_rng(61)
    pieces = [_random_pieces(rng, len(x), 200) for x in recs]
    runs = []
    for _ in range(2):
        _, ss = _segmenters(len(recs), 200, np.float32, 3, 2)
        runs.append(_feed(ss, _plan(recs, pieces), 1200, np.float32)[2])
    assert sum(len(t) for t, _, _ in runs[0]) >= 10
    for (t0, o0, n0), (t1, o1, n1) in zip(*runs):
        assert t0.tobytes() == t1.tobytes() and o0.tobytes() == o1.tobytes() and n0.tobytes() == n1.tobytes()


# ---- 8. errors -------------------------------------------------------------------------------------------------------------
def _raw_push(ss, cfg, samples, lengths, table, cap, total, state=None, state_bytes=None):
    return _native.lib().sir_stream_push(ss._handle, ss._state.data_ptr() if state is None else state,
                                         ss._state.numel() if state_bytes is None else state_bytes, C.byref(cfg), samples.data_ptr(),
                                         samples.stride(0), samples.shape[1], lengths.data_ptr(), None, None, table.data_ptr(), cap,
                                         total.data_ptr(), _native.current_stream_ptr())


def test_refused_calls_leave_the_state_alone_and_a_doctored_row_is_a_zero_row():
    P, n_stop, M = 1, 1, 12
    x = np.zeros((2, 1000), dtype=np.int16)
    for k in (1, 4, 7, 10):
        x[0, k * CH:(k + 1) * CH] = 4000 + k
        x[1, (k + 1) * CH:(k + 2) * CH] = -3000 - k
    _, ss = _segmenters(2, 1000, np.int16, P, n_stop, M=M)
    ss.reset()
    dx = torch.from_numpy(x).to(DEV)
    dl = torch.full((2,), 1000, dtype=torch.int32, device=DEV)
    table = torch.full((ss.max_rows + 1, 4), -7, dtype=torch.int64, device=DEV)
    total = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    cfg = ss.config()
    assert ss.max_rows == 2 * (16 + 2)

    def variant(**kw):
        c = ss.config()
        for k, v in kw.items():
            setattr(c.vad if k in ("chunk_size", "prior_chunks") else c, k, v)
        return c
    assert _raw_push(ss, cfg, dx, dl, table, ss.max_rows - 1, total) == _native.SIR_EINVAL         # table one row short
    assert b"seg_cap" in _native.lib().sir_last_error()
    assert _raw_push(ss, variant(ring_chunks=ss.min_ring_chunks - 1), dx, dl, table, ss.max_rows, total) == _native.SIR_EINVAL
    assert b"ring_chunks" in _native.lib().sir_last_error()
    assert _raw_push(ss, variant(max_utt_chunks=1), dx, dl, table, ss.max_rows, total) == _native.SIR_EINVAL     # M <= P
    assert b"max_utt_chunks" in _native.lib().sir_last_error()
    assert _raw_push(ss, variant(wave_dtype=7), dx, dl, table, ss.max_rows, total) == _native.SIR_EINVAL
    assert _raw_push(ss, variant(chunk_size=100), dx, dl, table, ss.max_rows, total) == _native.SIR_EINVAL
    assert _raw_push(ss, cfg, dx, dl, table, ss.max_rows, total, state=ss._state.data_ptr() + 16) == _native.SIR_EINVAL
    assert _raw_push(ss, cfg, dx, dl, table, ss.max_rows, total, state_bytes=ss._state.numel() - 256) == _native.SIR_ENOMEM
    assert _native.lib().sir_stream_state_bytes(ss._handle, C.byref(variant(ring_chunks=ss.min_ring_chunks - 1))) == 0
    torch.cuda.synchronize()
    assert int(total.item()) == -1 and (table == -7).all()         # nothing was launched
    # the same push with a full table: the state had not moved
    assert _raw_push(ss, cfg, dx, dl, table, ss.max_rows, total) == 0
    torch.cuda.synchronize()
    want = [[0, k * CH, (k + 2) * CH, 0] for k in (1, 4, 7, 10)] + [[1, (k + 1) * CH, (k + 3) * CH, 0] for k in (1, 4, 7, 10)]
    assert int(total.item()) == 8 and table[:8].cpu().numpy().tolist() == want
    assert (table[8:] == -7).all()                                  # rows at or beyond the total are not written
    good, tot = table[:8].clone(), total.clone()
    clips, lens = ss.gather(good, tot, 200)
    ref_clips, ref_len = vad_ref.gather(list(x), np.asarray(want)[:, :3], 200)
    assert np.array_equal(clips.cpu().numpy(), ref_clips) and np.array_equal(lens.cpu().numpy(), ref_len)
    ops.check_status()
    # doctored rows: a stream outside the slots, a reversed range, a range longer than the ring
    bad = good.clone()
    bad[1, 0] = 2
    bad[3, 1], bad[3, 2] = good[3, 2], good[3, 1]
    bad[5, 2] = bad[5, 1] + ss.ring_chunks * CH + 1
    clips, lens = ss.gather(bad, tot, 200)
    for s in (1, 3, 5):
        ref_clips[s] = 0.0
        ref_len[s] = 0
    assert np.array_equal(clips.cpu().numpy(), ref_clips) and np.array_equal(lens.cpu().numpy(), ref_len)
    with pytest.raises(_native.SirError, match="sir_stream_gather"):
        ops.check_status()
    ops.check_status()                                              # the word was cleared


# ---- 9. end to end ---------------------------------------------------------------------------------------------------------
def test_stream_session_end_to_end_equals_recognize_recordings():
    """the two recordings of test_vad_gpu.py::test_recognize_recordings_end_to_end at the listener's defaults (chunks of 1024), fed
    1000 samples at a time: same utterances, same labels, and logits bit-identical to the batch route's"""
    from sir_amd.scripts.testing import IntentRecognizer
    utt = synth.synth_clips(4, 40000, seed=77).numpy()
    z = lambda chunks: np.zeros(chunks * 1024, dtype=np.float32)
    rec0 = np.concatenate([z(8), utt[0, :24 * 1024], z(24), utt[1, :32 * 1024], z(20)])
    rec1 = np.concatenate([utt[2, :16 * 1024], z(32), utt[3, :5 * 1024], z(8)])
    recs = [rec0, rec1]
    torch.manual_seed(5)
    model = CNNAudioGRU(5).to(DEV).eval()
    label_map = {f"intent_{i}": i for i in range(5)}
    reco = IntentRecognizer.from_model(model, label_map, DEV)
    want = reco.recognize_recordings(recs, pad_to=200)
    assert [len(f) for f in want] == [2, 2]
    wave, wl = reco._load_group(recs)
    ref_table, ref_logits = reco.score_segments(wave, wl, pad_to=200)

    def stream_all(**kw):
        session = reco.open_streams(2, max_push=1000, pad_to=200, **kw)
        found, logits = [[], []], [[], []]
        for k in range(-(-max(len(r) for r in recs) // 1000)):
            chunks = {s: r[k * 1000:(k + 1) * 1000] for s, r in enumerate(recs) if k * 1000 < len(r)}
            close = [s for s, r in enumerate(recs) if k * 1000 < len(r) <= (k + 1) * 1000]
            for row, u in enumerate(session.feed(chunks, close=close)):
                found[u["stream"]].append(u)
                logits[u["stream"]].append(session.last_logits[row].cpu())
        return found, logits

    found, logits = stream_all()
    assert [len(f) for f in found] == [2, 2]
    flat = [u for f in found for u in f]
    assert [(u["stream"], round(u["start"] * SR), round(u["end"] * SR)) for u in flat] == [tuple(r) for r in ref_table.tolist()]
    for u, w in zip(flat, [w for f in want for w in f]):
        assert u["start"] == w["start"] and u["end"] == w["end"] and u["predicted_label"] == w["predicted_label"]
        assert u["forced"] is False
    got = torch.stack([row for rows in logits for row in rows])
    assert torch.equal(got, ref_logits)
    for u, w in zip(flat, [w for f in want for w in f]):
        assert {k: v for k, v in u.items() if k not in ("stream", "forced")} == w
    # the on-device result route, with a rejection threshold
    want = reco.recognize_recordings(recs, pad_to=200, on_device=True, min_confidence=0.5)
    found, _ = stream_all(on_device=True, min_confidence=0.5)
    for u, w in zip([u for f in found for u in f], [w for f in want for w in f]):
        assert "rejected" in u and {k: v for k, v in u.items() if k not in ("stream", "forced")} == w
    ops.check_status()
