"""GPU: the stream input stage (sir_stream_input_push, sir_amd.streaming.StreamInput) -- G.711 / int16 / float32 streams at the
caller's rate, decoded and rate-converted push by push -- alone, in front of StreamSegmenter and through IntentRecognizer.open_streams.

The contract under test is bit-equality: what a stream yields over its life is ``HipFeaturizer.resample`` (sir_resample) of the
whole decoded stream on the same handle, whatever the cut into pushes; every push emits exactly E(n_after) - E(n_before) outputs
(tests/stream_input_ref.py).  No tolerance is introduced here: the one inexact comparison, against the float64 evaluation, uses
tests/frontend_edge_ref.py's derived ``resample_bound``.

Streams are N = 2 (2 width + orig) + 37 input samples (67 at 8000 -> 16000, 987 at 44100 -> 16000) and, where that is below 300,
300 as well.  Measured on MI355X: every comparison here is exact and holds; the whole file runs in about 4 s, its slowest case (through
the recogniser, 135 feeds) in under 1 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import frontend_edge_ref as fe
import stream_input_ref as ref
import stream_ref
from sir_amd import _native, g711, ops, synth
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU
from sir_amd.streaming import StreamInput, StreamSegmenter

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.5
CASES = [(8000, 16000, "ulaw", np.uint8), (8000, 16000, "alaw", np.uint8), (44100, 16000, "pcm", np.int16),
         (48000, 16000, "pcm", np.float32), (11025, 16000, "pcm", np.float32), (16000, 8000, "pcm", np.int16)]
CASE_IDS = ["8k_ulaw", "8k_alaw", "44k1_i16", "48k_f32", "11k025_f32", "16k_to_8k_i16"]
TORCH_DT = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.float32): torch.float32}


def _signal(rng, n, enc, dtype, rate):
    """seeded noise plus a tone; random bytes for G.711"""
    if enc in ("ulaw", "alaw"):
        return rng.integers(0, 256, n, dtype=np.uint8)
    x = 0.2 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 440.0 * np.arange(n) / rate)
    if np.dtype(dtype) == np.int16:
        return np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)
    return x.astype(np.float32)


def _make(case, S, max_push):
    a, b, enc, dtype = case
    return StreamInput(S, max_push, a, b, encoding=enc, dtype=TORCH_DT[np.dtype(dtype)], device=DEV)


def _whole(xs, case):
    """sir_resample of whole decoded streams, one launch -> list of float32 arrays.  G.711 is decoded on the host (exact); int16 and
    float32 go in as they are (sir_resample dequantises int16 with the same s / 32768)."""
    a, b, enc, _ = case
    dec = [ref.decode(x, enc) if x.dtype == np.uint8 else x for x in xs]
    width = max(max(len(x) for x in dec), 1)
    host = np.zeros((len(dec), width), dtype=dec[0].dtype)
    for r, x in enumerate(dec):
        host[r, :len(x)] = x
    lens = torch.tensor([len(x) for x in dec], dtype=torch.int32, device=DEV)
    out, out_len = get_featurizer().resample(torch.from_numpy(host).to(DEV), a, b, lens)
    out, out_len = out.cpu().numpy(), out_len.cpu().numpy()
    return [out[r, :out_len[r]].copy() for r in range(len(dec))]


def _plan(x, pieces, close_last=True):
    at, ev = 0, []
    for k, m in enumerate(pieces):
        ev.append((x[at:at + m], close_last and k == len(pieces) - 1))
        at += m
    assert at == len(x)
    return ev


def _feed(si, plan, dtype):
    """plan[s]: the (samples, close) stream s hands over push by push.  -> (per stream the concatenated outputs, per stream the
    output count of every push it took part in).  Everything stays on the device until the plan is through."""
    S = si.n_streams
    outs, lens, took = [], [], []
    for k in range(max(len(ev) for ev in plan)):
        now = [ev[k] if k < len(ev) else (None, False) for ev in plan]
        width = max([1] + [len(x) for x, _ in now if x is not None])
        host = np.zeros((S, width), dtype=dtype)
        n = np.zeros(S, dtype=np.int32)
        for s, (x, _) in enumerate(now):
            if x is not None:
                host[s, :len(x)] = x
                n[s] = len(x)
        close = [s for s, (_, cl) in enumerate(now) if cl] or None
        out, out_len = si.push(torch.from_numpy(host).to(DEV), torch.from_numpy(n).to(DEV), close=close)
        assert out.shape == (S, si.max_out) and out_len.dtype == torch.int32
        outs.append(out)
        lens.append(out_len)
        took.append([x is not None for x, _ in now])
    lens = torch.stack(lens).cpu().numpy()
    outs = torch.stack(outs).cpu().numpy()
    assert lens.min() >= 0 and lens.max() <= si.max_out
    got = [np.concatenate([outs[k, s, :lens[k, s]] for k in range(len(lens))]) for s in range(S)]
    counts = [[int(lens[k, s]) for k in range(len(lens)) if took[k][s]] for s in range(S)]
    for k in range(len(lens)):
        for s in range(S):
            assert took[k][s] or lens[k, s] == 0                    # a stream that gets nothing emits nothing
    return got, counts


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _stream_lengths(t):
    n = t.stream_length()
    return [n] if n >= 300 else [n, 300]


# ---- 1. decode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_decode_all_codes_bit_for_bit(law):
    si = StreamInput(4, 300, 8000, 8000, encoding=law, device=DEV)
    assert si.max_out == 300
    codes = np.arange(256, dtype=np.uint8)
    want = (ref.expand(codes, law).astype(np.float64) / 32768.0).astype(np.float32)
    for b, v in ref.ANCHORS[law].items():
        assert want[b] == np.float32(v / 32768.0)
    host = np.full((4, 300), 0x5A, dtype=np.uint8)
    host[0, :256] = codes
    host[2, :256] = codes[::-1]
    lens = torch.tensor([256, 0, 17, 0], dtype=torch.int32, device=DEV)
    for _ in range(2):                                              # twice: the second push finds n = 256 / 17 in the state
        out = torch.full((4, 300), SENTINEL, dtype=torch.float32, device=DEV)
        got, got_len = si.push(torch.from_numpy(host).to(DEV), lens, out=out)
        assert got is out
        got, got_len = got.cpu().numpy(), got_len.cpu().numpy()
        assert got_len.tolist() == [256, 0, 17, 0]
        assert np.array_equal(_bits(got[0, :256]), _bits(want)) and np.array_equal(_bits(got[2, :17]), _bits(want[::-1][:17]))
        assert (got[0, 256:] == SENTINEL).all() and (got[2, 17:] == SENTINEL).all() and (got[[1, 3]] == SENTINEL).all()
    assert np.array_equal(want, g711.table(law).astype(np.float32) / 32768.0)
    ops.check_status()


# ---- 2. cut invariance and equality with sir_resample ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_any_cut_equals_sir_resample_of_the_whole_stream(case):
    a, b, enc, dtype = case
    t = ref.Table(a, b)
    for total in _stream_lengths(t):
        rng = np.random.default_rng(a + 7 * b + total)
        x = _signal(rng, total, enc, dtype, a)
        want = _whole([x], case)[0]
        assert len(want) == t.out_len(total) == _native.lib().sir_resample_out_len(total, a, b)
        y, S = fe.resample64(ref.decode(x, enc).astype(np.float64), a, b)
        assert (np.abs(want - y) <= fe.resample_bound(S, a, b)).all()
        max_in = max(t.orig, 3) + 5
        plans = dict(ref.schedules(t, total, max_in, seed=total))
        plans["all"] = [total]
        assert len(plans) == 5
        for name, pieces in plans.items():
            si = _make(case, 1, total if name == "all" else max_in)
            assert si.max_out == t.max_out(si.max_push)
            got, counts = _feed(si, [_plan(x, pieces)], dtype)
            assert counts[0] == ref.counts(t, pieces), name          # every push: E(n_after) - E(n_before); the close: the rest
            assert sum(counts[0]) == len(want) and max(counts[0]) <= si.max_out
            assert np.array_equal(_bits(got[0]), _bits(want)), name
            assert (np.abs(got[0] - y) <= fe.resample_bound(S, a, b)).all(), name
    ops.check_status()


# ---- 3. independence and slot reuse ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=[CASE_IDS[0], CASE_IDS[2]])
def test_300_streams_are_independent_and_a_reused_slot_starts_fresh(case):
    a, b, enc, dtype = case
    S, max_in = 300, 100
    rng = np.random.default_rng(300 + a)
    first = [_signal(rng, int(n), enc, dtype, a) for n in rng.integers(0, 701, S)]
    first[7], first[256] = first[7][:0], _signal(rng, 700, enc, dtype, a)          # an empty caller; a full one behind the tile edge
    second = {s: _signal(rng, int(rng.integers(1, 400)), enc, dtype, a) for s in range(0, S, 5)}

    def pieces_of(x):
        out, left = [], len(x)
        while left > 0:
            m = min(left, int(rng.integers(0, max_in + 1)))
            out.append(m)
            left -= m
        return out or [0]
    plan = []
    for s in range(S):
        ev = _plan(first[s], pieces_of(first[s]))                   # closed with its last samples, mid-way through the run
        if s in second:
            ev += _plan(second[s], pieces_of(second[s]))            # the slot's next caller: a different signal from position 0
        plan.append(ev)
    runs = [_feed(_make(case, S, max_in), plan, dtype) for _ in range(2)]
    got = runs[0][0]
    for s in range(S):
        assert got[s].tobytes() == runs[1][0][s].tobytes() and runs[0][1][s] == runs[1][1][s]          # two runs, identical bits
    want_a = _whole(first, case)
    want_b = dict(zip(second, _whole([second[s] for s in second], case)))
    for s in range(S):
        want = np.concatenate([want_a[s], want_b[s]]) if s in second else want_a[s]
        assert np.array_equal(_bits(got[s]), _bits(want)), s
    # single-stream runs on a fresh state (test 2's code path): the same bits, for the reused slots and across the 256-stream edge
    for s in (0, 5, 7, 255, 256, 295, 299):
        lives = [first[s]] + ([second[s]] if s in second else [])
        alone = [_feed(_make(case, 1, max_in), [_plan(x, pieces_of(x))], dtype)[0][0] for x in lives]
        assert np.array_equal(_bits(np.concatenate(alone)), _bits(got[s])), s
    ops.check_status()


# ---- 4. max_out is a bound and is needed; 5. refusals ------------------------------------------------------------------------------
def _raw_push(si, cfg, samples, lengths, out, out_len, out_stride=None, state=None, state_bytes=None, in_width=None, in_stride=None,
              null=()):
    p = lambda name, v: None if name in null else v
    return _native.lib().sir_stream_input_push(
        p("h", si._handle), p("state", si._state.data_ptr() if state is None else state), si._state.numel() if state_bytes is None else state_bytes,
        C.byref(cfg) if "cfg" not in null else None, p("in", samples.data_ptr()), samples.stride(0) if in_stride is None else in_stride,
        samples.shape[1] if in_width is None else in_width, p("lengths", lengths.data_ptr()), None, p("out", out.data_ptr()),
        out.stride(0) if out_stride is None else out_stride, p("out_len", out_len.data_ptr()), _native.current_stream_ptr())


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_max_out_is_a_bound_and_one_column_less_is_refused(case):
    a, b, enc, dtype = case
    t = ref.Table(a, b)
    total = max(t.stream_length(), 300)
    rng = np.random.default_rng(4 + a + b)
    x = _signal(rng, total, enc, dtype, a)
    want = _whole([x], case)[0]
    max_in = max(t.orig, 3) + 5
    pieces = ref.schedules(t, total, max_in, seed=9)["max"]
    half = len(pieces) // 2
    si = _make(case, 1, max_in)
    assert _native.lib().sir_stream_input_max_out(C.byref(si.config())) == si.max_out == t.max_out(max_in)
    head, counts_head = _feed(si, [_plan(x[:sum(pieces[:half])], pieces[:half], close_last=False)], dtype)
    # one column short: refused before anything is launched
    at = sum(pieces[:half])
    row = torch.from_numpy(x[at:at + pieces[half]][None, :].copy()).to(DEV)
    n = torch.tensor([pieces[half]], dtype=torch.int32, device=DEV)
    out = torch.full((1, si.max_out), SENTINEL, dtype=torch.float32, device=DEV)
    out_len = torch.full((1,), -3, dtype=torch.int32, device=DEV)
    before = si._state.clone()
    assert _raw_push(si, si.config(), row, n, out, out_len, out_stride=si.max_out - 1) == _native.SIR_EINVAL
    assert b"out_stride" in _native.lib().sir_last_error()
    torch.cuda.synchronize()
    assert torch.equal(si._state, before) and (out == SENTINEL).all() and int(out_len.item()) == -3
    # the stream goes on as if the refused call had not been made
    tail, counts_tail = _feed(si, [_plan(x[at:], pieces[half:])], dtype)
    assert np.array_equal(_bits(np.concatenate([head[0], tail[0]])), _bits(want))
    assert counts_head[0] + counts_tail[0] == ref.counts(t, pieces)
    assert max(counts_head[0] + counts_tail[0]) <= si.max_out
    ops.check_status()


def test_refused_calls_write_nothing_and_leave_the_state_alone():
    case = CASES[0]
    si = _make(case, 3, 200)
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (3, 200), dtype=np.uint8)
    si.push(torch.from_numpy(x).to(DEV))                            # some state to lose
    lib = _native.lib()
    row = torch.from_numpy(x).to(DEV)
    n = torch.full((3,), 200, dtype=torch.int32, device=DEV)
    out = torch.full((3, si.max_out), SENTINEL, dtype=torch.float32, device=DEV)
    out_len = torch.full((3,), -3, dtype=torch.int32, device=DEV)
    before = si._state.clone()

    def variant(**kw):
        c = si.config()
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    E, M = _native.SIR_EINVAL, _native.SIR_ENOMEM
    cfg = si.config()
    for name in ("h", "state", "cfg", "in", "lengths", "out", "out_len"):
        assert _raw_push(si, cfg, row, n, out, out_len, null=(name,)) == E, name
    for kw in (dict(in_dtype=4), dict(in_dtype=-1), dict(in_rate=0), dict(in_rate=-8000), dict(out_rate=0), dict(n_streams=0),
               dict(n_streams=65536), dict(max_in=0), dict(max_in=(1 << 24) + 1), dict(max_in=199)):       # (199: in_width above max_in)
        assert _raw_push(si, variant(**kw), row, n, out, out_len) == E, kw
    assert _raw_push(si, cfg, row, n, out, out_len, in_width=0) == E
    assert _raw_push(si, cfg, row, n, out, out_len, in_width=201) == E
    assert _raw_push(si, cfg, row, n, out, out_len, in_stride=199) == E
    assert _raw_push(si, cfg, row, n, out, out_len, state=si._state.data_ptr() + 16) == E
    assert _raw_push(si, cfg, row, n, out, out_len, out_stride=si.max_out - 1) == E
    big = variant(in_rate=1, out_rate=48000, max_in=1 << 24)
    assert lib.sir_stream_input_max_out(C.byref(big)) == -1 and lib.sir_stream_input_state_bytes(si._handle, C.byref(big)) == 0
    assert _raw_push(si, big, row, n, out, out_len) == E            # a max_out that does not fit an int
    assert _raw_push(si, cfg, row, n, out, out_len, state_bytes=si._state.numel() - 256) == M
    assert lib.sir_stream_input_reset(si._handle, si._state.data_ptr(), si._state.numel() - 256, C.byref(cfg), None, _native.current_stream_ptr()) == M
    assert lib.sir_stream_input_reset(si._handle, si._state.data_ptr() + 16, si._state.numel(), C.byref(cfg), None, _native.current_stream_ptr()) == E
    assert lib.sir_stream_input_reset(si._handle, si._state.data_ptr(), si._state.numel(), C.byref(variant(in_dtype=9)), None,
                                      _native.current_stream_ptr()) == E
    assert lib.sir_stream_input_state_bytes(si._handle, C.byref(cfg)) == si._state.numel() > 0
    assert lib.sir_stream_input_state_bytes(si._handle, C.byref(variant(in_dtype=4))) == 0
    torch.cuda.synchronize()
    assert torch.equal(si._state, before) and (out == SENTINEL).all() and (out_len == -3).all()
    # the other entry points keep refusing the G.711 dtypes
    fz = get_featurizer()
    wave = torch.zeros((1, 4096), dtype=torch.float32, device=DEV)
    one = torch.tensor([4096], dtype=torch.int32, device=DEV)
    res = torch.full((1, 8192), SENTINEL, dtype=torch.float32, device=DEV)
    feats = torch.full((1, 64, 16), SENTINEL, dtype=torch.float32, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    vad = _native.VadConfig(1024, 0.01, 16, 7, 1)
    for dt in (_native.WAVE_ULAW, _native.WAVE_ALAW):
        assert lib.sir_resample(fz.handle, wave.data_ptr(), dt, 4096, one.data_ptr(), 1, 4096, 8000, 16000, res.data_ptr(), 8192, 8192,
                                None, _native.current_stream_ptr()) == E
        assert lib.sir_stream_state_bytes(fz.handle, C.byref(_native.StreamConfig(vad, 1, dt, 1024, 100, 200))) == 0
        assert lib.sir_features_fwd(fz.handle, wave.data_ptr(), dt, 4096, one.data_ptr(), 1, 4096, feats.data_ptr(), 16, None,
                                    ws.data_ptr(), ws.numel(), None, _native.current_stream_ptr()) == E
    assert lib.sir_stream_state_bytes(fz.handle, C.byref(_native.StreamConfig(vad, 1, _native.WAVE_F32, 1024, 100, 200))) > 0
    torch.cuda.synchronize()
    assert (res == SENTINEL).all() and (feats == SENTINEL).all()
    # and the stream that was refused all this continues from where it was
    got, got_len = si.push(row, n, close=[0, 1, 2])
    both = np.concatenate([x, x], axis=1)
    want = _whole(list(both), case)
    t = ref.Table(case[0], case[1])
    got, got_len = got.cpu().numpy(), got_len.cpu().numpy()
    for s in range(3):
        assert got_len[s] == t.out_len(400) - t.emitted(200)
        assert np.array_equal(_bits(got[s, :got_len[s]]), _bits(want[s][t.emitted(200):])), s
    ops.check_status()


# ---- 6. through the segmenter ------------------------------------------------------------------------------------------------------
def _telephone_recording():
    """8 kHz mu-law, 4 s: three bursts of a 0.3-amplitude 440 Hz tone on the 16 kHz detector's 256-sample chunk grid (128 input
    samples), more than the silence limit (1 s) of code 0xFF -- which decodes to exactly 0 -- between them"""
    rate, grid = 8000, 128
    x = np.full(4 * rate, 0xFF, dtype=np.uint8)
    bursts = [(12 * grid, 37 * grid), (110 * grid, 135 * grid), (210 * grid, 230 * grid)]
    for a, b in bursts:
        tone = 0.3 * np.sin(2 * np.pi * 440.0 * np.arange(b - a) / rate)
        x[a:b] = g711.encode(np.round(tone * 32767.0).astype(np.int16), "ulaw")
        assert b - a > 0 and a % grid == 0 and b % grid == 0
    for (_, b), (a, _) in zip(bursts[:-1], bursts[1:]):
        assert a - b > rate
    assert (ref.decode(x[:bursts[0][0]], "ulaw") == 0).all()
    return x


def _segment_all(ss, x, pieces, dtype, max_clip):
    rows, clips = [], []
    at = 0
    for k, m in enumerate(pieces):
        chunk = torch.from_numpy(x[at:at + m][None, :].copy()).to(DEV) if m else torch.zeros((1, 1), dtype=TORCH_DT[np.dtype(dtype)], device=DEV)
        n = torch.tensor([m], dtype=torch.int32, device=DEV)
        out, out_len, table = ss.push(chunk, n, close=[0] if k == len(pieces) - 1 else None, max_clip_len=max_clip)
        at += m
        tb, o, ol = table.cpu().numpy(), out.cpu().numpy(), out_len.cpu().numpy()
        for r, row in enumerate(tb):
            rows.append(tuple(int(v) for v in row))
            clips.append(o[r, :ol[r]].copy())
    assert at == len(x)
    return rows, clips


def test_through_the_segmenter_equals_the_detector_on_the_resampled_recording():
    x = _telephone_recording()
    case = (8000, 16000, "ulaw", np.uint8)
    x16 = _whole([x], case)[0]
    assert len(x16) == 64000
    kw = dict(device=DEV, chunk_size=256)
    plain = StreamSegmenter(1, 1024, dtype=torch.float32, **kw)
    max_clip = 40000
    want_rows, want_clips = _segment_all(plain, x16, [1024] * 62 + [512], np.float32, max_clip)
    assert len(want_rows) == 3                                      # the equality below cannot pass empty
    # the numpy detector on a float64 evaluation of the same conversion finds the same three (no decision hinges on a rounding:
    # a chunk is all tone, mean |x| = 0.19, or filter ringing far below the threshold)
    y, _ = fe.resample64(ref.decode(x, "ulaw").astype(np.float64), 8000, 16000)
    host_rows = stream_ref.run(y.astype(np.float32), [len(y)], 256, plain.threshold, plain.prior_chunks, plain.silence_chunks, plain.max_utt_chunks)
    assert len(host_rows) == 3 and [r[1:] for r in want_rows] == host_rows
    rng = np.random.default_rng(6)
    rand, left = [], len(x)
    while left > 0:
        rand.append(min(left, int(rng.integers(0, 1001))))
        left -= rand[-1]
    for max_push, pieces in ((400, [400] * 80), (1000, rand), (1000, [1000] * 32)):
        ss = StreamSegmenter(1, max_push, input_rate=8000, encoding="ulaw", **kw)
        assert ss.input is not None and ss.dtype == torch.uint8
        rows, clips = _segment_all(ss, x, pieces, np.uint8, max_clip)
        assert rows == want_rows
        assert len(clips) == 3 and all(np.array_equal(_bits(c), _bits(w)) for c, w in zip(clips, want_clips))
    for (s, a, b, _), clip in zip(want_rows, want_clips):
        assert np.array_equal(_bits(clip), _bits(x16[a:b]))
    ops.check_status()


# ---- 7. through the recogniser -----------------------------------------------------------------------------------------------------
def test_open_streams_on_alaw_telephony_equals_recognize_recordings():
    from sir_amd.scripts.testing import IntentRecognizer
    utt = synth.synth_clips(4, 20000, seed=78).numpy()              # taken as 8 kHz material: 2.5 s each
    enc = lambda v: g711.encode(np.round(np.clip(v, -1.0, 1.0) * 32767.0).astype(np.int16), "alaw")
    z = lambda n: np.full(n, 0xD5, dtype=np.uint8)                  # A-law has no zero: +8 / 32768, far below the threshold
    rec0 = np.concatenate([z(4000), enc(utt[0, :12000]), z(12000), enc(utt[1, :16000]), z(10000)])
    rec1 = np.concatenate([enc(utt[2, :8000]), z(16000), enc(utt[3, :3200]), z(4000)])
    recs = [rec0, rec1]
    case = (8000, 16000, "alaw", np.uint8)
    recs16 = _whole(recs, case)
    model = CNNAudioGRU(5)
    model.load_state_dict(synth.synth_state_dict(5, seed=3))
    reco = IntentRecognizer.from_model(model.to(DEV).eval(), {f"intent_{i}": i for i in range(5)}, DEV)
    want = reco.recognize_recordings(recs16, pad_to=200)
    assert [len(f) for f in want] == [2, 2]
    wave, wl = reco._load_group(recs16)
    ref_table, ref_logits = reco.score_segments(wave, wl, pad_to=200)
    session = reco.open_streams(2, max_push=400, pad_to=200, sample_rate=8000, encoding="alaw")
    found, logits = [[], []], [[], []]
    for k in range(-(-max(len(r) for r in recs) // 400)):
        chunks = {s: (r[k * 400:(k + 1) * 400].tobytes() if s == 0 else r[k * 400:(k + 1) * 400])       # bytes and uint8 arrays alike
                  for s, r in enumerate(recs) if k * 400 < len(r)}
        close = [s for s, r in enumerate(recs) if k * 400 < len(r) <= (k + 1) * 400]
        for row, u in enumerate(session.feed(chunks, close=close)):
            found[u["stream"]].append(u)
            logits[u["stream"]].append(session.last_logits[row].cpu())
    assert [len(f) for f in found] == [2, 2]
    flat = [u for f in found for u in f]
    assert [(u["stream"], round(u["start"] * 16000), round(u["end"] * 16000)) for u in flat] == [tuple(r) for r in ref_table.tolist()]
    assert torch.equal(torch.stack([row for rows in logits for row in rows]), ref_logits)
    for u, w in zip(flat, [w for f in want for w in f]):
        assert u["forced"] is False and {k: v for k, v in u.items() if k not in ("stream", "forced")} == w
    ops.check_status()
