"""GPU: utterance segmentation of long recordings (sir_vad_segment / sir_vad_gather, sir_amd.segmenter, sir_amd.scripts.testing)
against the numpy reference tests/vad_ref.py.

Shapes.  The kernels have seams at 32 chunks (one flag word = one thread of the segmentation scan, one wave of the energy
kernel), at 2048 chunks (64 words = one wave of the scan) and at 8192 chunks (256 words = one tile of the block; state is carried
from tile to tile).  With chunk_size = 64 one batch therefore holds recordings of 1, 63, 64, 65, 255, 256, 257, 1025, 2049 and
8193 chunks plus an empty one, with trailing partial chunks of 1 and of 63 samples; the samples behind a recording's length are
loud, so a read past the length would turn silence into speech.

Energies.  int16: bit-identical to float32(S / (count * 32768)).  float32: the kernel adds, per accumulator, chunk_size / 64
values in a chain (the first addition, to 0, is exact), joins its four accumulators in 2 levels and 16 lanes in 4 levels, then
divides once: at most k = chunk_size / 64 + 6 roundings on any path.  All terms are non-negative, so every rounding error is
relative to a partial sum that is <= the final sum, and the result is within gamma_k = k u / (1 - k u), u = 2^-24, of the exact
mean, relative (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); the float64 reference's own error (~1e-16)
is three orders below and is absorbed by evaluating the bound with k + 1.  Waves are built so that every chunk's energy is
<= threshold / 2 or >= 2 * threshold (asserted on the reference energies): no decision can hinge on a rounding.

Measured on MI355X: not yet -- this file was written without a GPU at hand; test_energy_f32_* prints its worst error when run.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import vad_ref
from sir_amd import _native, ops, synth
from sir_amd.featurizer import HOP, get_featurizer
from sir_amd.models.models import CNNAudioGRU
from sir_amd.segmenter import Segmenter

pytestmark = pytest.mark.gpu
DEV = "cuda"
CH = 64
THR = 0.01
CHUNKS = [1, 63, 64, 65, 255, 256, 257, 1025, 2049, 8193, 0]
PARTIAL = {3: 1, 4: 63, 9: 17}                     # recording -> samples of its trailing partial chunk
LENGTHS = [n * CH - (CH - PARTIAL[r] if r in PARTIAL else 0) for r, n in enumerate(CHUNKS)]
MAX_LEN = -(-max(LENGTHS) // 8) * 8
U = 2.0 ** -24


def _make_waves(density, dtype, c=CH, lengths=LENGTHS, max_len=MAX_LEN, seed=0):
    """[n_rec, max_len] waves whose chunks are speech with probability `density`: |x| in [2.5, 50] * THR on speech chunks,
    <= 0.4 * THR on silent ones, and 0.9 behind every recording's length"""
    rng = np.random.default_rng(1000 + seed + int(density * 100))
    n_rec = len(lengths)
    x = np.full((n_rec, max_len), 0.9, dtype=np.float64)
    for r, length in enumerate(lengths):
        n = vad_ref.n_chunks(length, c)
        speech = rng.random(n) < density
        amp = np.where(speech, rng.uniform(2.5 * THR, 50 * THR, n), rng.uniform(0.0, 0.4 * THR, n))
        lo = np.where(speech, 2.5 * THR, 0.0)
        mag = lo.repeat(c) + (amp - lo).repeat(c) * rng.random(n * c)
        sign = rng.integers(0, 2, n * c) * 2 - 1
        x[r, :length] = (mag * sign)[:length]
    if dtype == np.int16:
        return np.round(x * 32767.0).astype(np.int16)
    return x.astype(np.float32)


_cache = {}


def _case(density, dtype, c=CH, lengths=tuple(LENGTHS), max_len=MAX_LEN):
    """(host waves, device waves, device lengths, reference energies, reference flags), built once per key"""
    key = (density, np.dtype(dtype).name, c, lengths, max_len)
    if key not in _cache:
        w = _make_waves(density, dtype, c, list(lengths), max_len)
        energies = [vad_ref.chunk_energy(w[r], n, c) for r, n in enumerate(lengths)]
        flags = [e.astype(np.float32) > np.float32(THR) for e in energies]
        _cache[key] = (w, torch.from_numpy(w).to(DEV), torch.tensor(lengths, dtype=torch.int32, device=DEV), energies, flags)
    return _cache[key]


def _cfg(c=CH, thr=THR, n_stop=16, prior=7, flush=1):
    return _native.VadConfig(c, thr, n_stop, prior, flush)


def _segment_raw(wave, lengths, cfg, seg_cap, want_energy=False, guard_rows=0, ws_bytes=None, max_len=None):
    """one sir_vad_segment call -> (rc, table [seg_cap + guard_rows, 3] prefilled with -7, seg_count, total, energy)"""
    lib = _native.lib()
    h = get_featurizer().handle
    n_rec = wave.shape[0]
    max_len = wave.shape[1] if max_len is None else max_len
    dt = _native.WAVE_I16 if wave.dtype == torch.int16 else _native.WAVE_F32
    table = torch.full((seg_cap + guard_rows, 3), -7, dtype=torch.int32, device=DEV)
    seg_count = torch.full((n_rec,), -1, dtype=torch.int32, device=DEV)
    total = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    need = lib.sir_vad_workspace_bytes(h, n_rec, max_len, cfg.chunk_size)
    ws = torch.full((max(need, 256),), 0xA5, dtype=torch.uint8, device=DEV)
    energy = torch.full((n_rec, -(-max_len // cfg.chunk_size)), -1.0, dtype=torch.float32, device=DEV) if want_energy else None
    rc = lib.sir_vad_segment(h, wave.data_ptr(), dt, wave.stride(0), lengths.data_ptr(), n_rec, max_len, C.byref(cfg),
                             energy.data_ptr() if want_energy else None, seg_count.data_ptr(), table.data_ptr(), seg_cap,
                             total.data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes, _native.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, table.cpu().numpy(), seg_count.cpu().numpy(), int(total.item()), energy.cpu().numpy() if want_energy else None


def _gather_raw(wave, table, total, seg_cap, max_clip, out_stride=None, n_rec=None):
    """one sir_vad_gather call on outputs prefilled with a guard -> (rc, out [seg_cap, out_stride], out_lengths)"""
    lib = _native.lib()
    out_stride = max_clip + 8 if out_stride is None else out_stride
    out = torch.full((seg_cap, out_stride), 77.0, dtype=torch.float32, device=DEV)
    out_len = torch.full((seg_cap,), -3, dtype=torch.int32, device=DEV)
    dt = _native.WAVE_I16 if wave.dtype == torch.int16 else _native.WAVE_F32
    t = torch.as_tensor(table, dtype=torch.int32).to(DEV).contiguous()
    tot = torch.tensor([total], dtype=torch.int32, device=DEV)
    rc = lib.sir_vad_gather(get_featurizer().handle, wave.data_ptr(), dt, wave.stride(0), wave.shape[0] if n_rec is None else n_rec,
                            t.data_ptr(), tot.data_ptr(), seg_cap, out.data_ptr(), out.stride(0), max_clip, out_len.data_ptr(),
                            _native.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), out_len.cpu().numpy()


def test_energy_i16_is_the_correctly_rounded_mean():
    w, dw, dl, energies, flags = _case(0.5, np.int16)
    rc, _, _, _, e = _segment_raw(dw, dl, _cfg(), 0, want_energy=True)
    assert rc == 0
    for r, ref in enumerate(energies):
        assert np.array_equal(e[r, :len(ref)], ref.astype(np.float32)), r
        assert not e[r, len(ref):].any(), r                         # zero behind the recording's own chunks


def test_energy_threshold_is_strict():
    """a chunk of all |s| = 256 has energy 2^-7 exactly: not speech at threshold 2^-7; one sample at 257 makes it speech"""
    x = np.full((2, 3 * CH), 256, dtype=np.int16)
    x[:, ::2] *= -1
    x[1, CH + 5] = 257
    dw = torch.from_numpy(x).to(DEV)
    dl = torch.tensor([3 * CH, 3 * CH], dtype=torch.int32, device=DEV)
    rc, table, count, total, e = _segment_raw(dw, dl, _cfg(thr=2.0 ** -7, n_stop=0, prior=0), 8, want_energy=True)
    assert rc == 0
    assert e[0].tolist() == [2.0 ** -7] * 3 and e[1, 0] == 2.0 ** -7 and e[1, 1] > 2.0 ** -7
    assert count.tolist() == [0, 1] and total == 1
    assert table[0].tolist() == [1, CH, 2 * CH]


@pytest.mark.parametrize("c", [64, 1024])
def test_energy_f32_within_the_bound_of_its_own_additions(c):
    lengths = tuple(LENGTHS) if c == 64 else (40 * 1024 + 500, 75 * 1024, 100 * 1024 + 1)
    max_len = MAX_LEN if c == 64 else 100 * 1024 + 8
    w, dw, dl, energies, flags = _case(0.5, np.float32, c, lengths, max_len)
    rc, _, _, _, e = _segment_raw(dw, dl, _cfg(c=c), 0, want_energy=True)
    assert rc == 0
    k = c // 64 + 6 + 1
    gamma = k * U / (1 - k * U)
    worst = 0.0
    for r, ref in enumerate(energies):
        assert ((ref <= THR / 2) | (ref >= 2 * THR)).all()          # the margin that keeps decisions off the rounding
        err = np.abs(e[r, :len(ref)].astype(np.float64) - ref)
        worst = max(worst, float((err / ref.clip(min=1e-300)).max()) if len(ref) else 0.0)
        assert (err <= gamma * ref).all(), (r, worst, gamma)
    print(f"chunk {c}: worst relative error {worst:.3e}, bound {gamma:.3e}")


@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["i16", "f32"])
@pytest.mark.parametrize("density", [0.05, 0.2, 0.5, 0.9])
def test_table_equals_the_reference(density, dtype):
    w, dw, dl, energies, flags = _case(density, dtype)
    for e in energies:
        assert ((e <= THR / 2) | (e >= 2 * THR)).all()
    for prior, n_stop, flush in itertools.product((0, 1, 7), (0, 1, 16), (1, 0)):
        counts, ref = vad_ref.segment_batch(w, LENGTHS, CH, THR, prior, n_stop, bool(flush), flags=flags)
        cap = len(ref) + 3
        rc, table, seg_count, total, _ = _segment_raw(dw, dl, _cfg(n_stop=n_stop, prior=prior, flush=flush), cap)
        assert rc == 0
        assert total == len(ref), (prior, n_stop, flush)
        assert np.array_equal(seg_count, counts), (prior, n_stop, flush)
        assert np.array_equal(table[:total], ref), (prior, n_stop, flush)
        assert (table[total:] == -7).all()


def test_unaligned_rows_take_the_scalar_path():
    """a wave whose rows start 2 bytes off a 16-byte boundary: same table, same energies"""
    w, dw, dl, energies, flags = _case(0.2, np.int16)
    big = torch.zeros((dw.shape[0], dw.shape[1] + 8), dtype=torch.int16, device=DEV)
    view = big[:, 1:1 + dw.shape[1]]
    view.copy_(dw)
    assert view.data_ptr() % 16 != 0
    counts, ref = vad_ref.segment_batch(w, LENGTHS, CH, THR, 7, 16, True, flags=flags)
    rc, table, seg_count, total, e = _segment_raw(view, dl, _cfg(), len(ref), want_energy=True)
    assert rc == 0 and total == len(ref) and np.array_equal(table, ref) and np.array_equal(seg_count, counts)
    for r, en in enumerate(energies):
        assert np.array_equal(e[r, :len(en)], en.astype(np.float32))
    rc, out, out_len = _gather_raw(view, ref, total, total, 200)
    want, want_len = vad_ref.gather(w, ref, 200)
    assert rc == 0 and np.array_equal(out[:, :200], want) and np.array_equal(out_len, want_len)


def test_listener_defaults_at_chunk_1024():
    lengths = (40 * 1024 + 500, 75 * 1024, 100 * 1024 + 1)
    seg = Segmenter()
    assert (seg.chunk_size, seg.prior_chunks, seg.silence_chunks) == (1024, 7, 16)
    for dtype in (np.int16, np.float32):
        w, dw, dl, energies, flags = _case(0.05, dtype, 1024, lengths, 100 * 1024 + 8)
        counts, ref = vad_ref.segment_batch(w, lengths, 1024, THR, 7, 16, True, flags=flags)
        assert len(ref) >= 3
        table, seg_count, total = seg.segment(dw, dl)
        assert int(total.item()) == len(ref)
        assert np.array_equal(table.cpu().numpy(), ref) and np.array_equal(seg_count.cpu().numpy(), counts)
        clips, clip_lens, _ = seg.clips(dw, dl, max_clip_len=30000)
        want, want_len = vad_ref.gather(w, ref, 30000)
        assert np.array_equal(clips.cpu().numpy(), want) and np.array_equal(clip_lens.cpu().numpy(), want_len)
    ops.check_status()


def test_table_smaller_than_the_total():
    w, dw, dl, energies, flags = _case(0.2, np.int16)
    counts, ref = vad_ref.segment_batch(w, LENGTHS, CH, THR, 1, 1, True, flags=flags)
    cap = len(ref) // 2
    assert cap >= 8
    rc, table, seg_count, total, _ = _segment_raw(dw, dl, _cfg(n_stop=1, prior=1), cap, guard_rows=64)
    assert rc == 0
    assert total == len(ref) and np.array_equal(seg_count, counts)         # the true counts
    assert np.array_equal(table[:cap], ref[:cap])
    assert (table[cap:] == -7).all()                                        # nothing behind the table was touched
    # the Segmenter regrows: a capacity far below the total still returns the whole table
    seg = Segmenter(chunk_size=CH, silence_limit=0.5 * CH / 16000, prior_recording=1.5 * CH / 16000)
    assert (seg.silence_chunks, seg.prior_chunks) == (1, 1)
    seg.initial_seg_cap = 4
    short = [min(n, 4096) for n in LENGTHS]
    _, ref = vad_ref.segment_batch(w[:, :4096], short, CH, THR, 1, 1, True)
    assert len(ref) > 4
    t, _, tot = seg.segment(dw[:, :4096], torch.tensor(short, dtype=torch.int32, device=DEV))
    assert int(tot.item()) == len(ref) and np.array_equal(t.cpu().numpy(), ref)


@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["i16", "f32"])
def test_gather(dtype):
    w, dw, dl, energies, flags = _case(0.2, dtype)
    _, ref = vad_ref.segment_batch(w, LENGTHS, CH, THR, 2, 1, True, flags=flags)      # short segments, many rows
    total = len(ref)
    longest = int((ref[:, 2] - ref[:, 1]).max())
    for max_clip in (100, longest, 1003):                                   # cut most rows / cut none / wider than any, odd width
        cap = total + 5
        rc, out, out_len = _gather_raw(dw, np.concatenate([ref, np.full((5, 3), 1 << 30, np.int32)]), total, cap, max_clip)
        assert rc == 0
        want, want_len = vad_ref.gather(w, ref, max_clip)
        assert np.array_equal(out[:total, :max_clip], want)                 # samples, truncation, zero tails
        assert np.array_equal(out_len[:total], want_len)
        assert (out[:total, max_clip:] == 77.0).all()                       # nothing behind max_clip_len
        assert (out[total:] == 77.0).all() and not out_len[total:].any()    # rows at or beyond total: length 0 only
    ops.check_status()                                                      # the rows beyond total were never looked at
    # hand-written rows (the segmenter only ever starts a clip on a chunk boundary): an aligned start with whole 16-byte groups,
    # starts off the 16-byte grid, an aligned start whose clip ends inside a group, a clip cut at max_clip_len, an empty clip;
    # into aligned output rows whose last group is partial (203 of 208) and into rows no vector store may touch (201 apart)
    hand = np.array([[5, 64, 256], [6, 3, 203], [7, 128, 165], [8, 130, 430], [9, 8, 8], [5, 321, 322]], dtype=np.int32)
    for max_clip, out_stride in ((203, 208), (200, 201)):
        rc, out, out_len = _gather_raw(dw, hand, len(hand), len(hand) + 2, max_clip, out_stride=out_stride)
        assert rc == 0
        want, want_len = vad_ref.gather(w, hand, max_clip)
        assert want_len.tolist() == [192, 200, 37, max_clip, 0, 1]
        assert np.array_equal(out[:len(hand), :max_clip].view(np.uint32), want.view(np.uint32))
        assert np.array_equal(out_len[:len(hand)], want_len) and not out_len[len(hand):].any()
        assert (out[:len(hand), max_clip:] == 77.0).all() and (out[len(hand):] == 77.0).all()
    ops.check_status()
    # corrupted rows: a recording outside the batch, a reversed range, a range past the row -> zero rows + SIR_EINVAL
    bad = ref.copy()
    bad[1, 0] = len(LENGTHS)
    bad[3, 1], bad[3, 2] = bad[3, 2] + 64, bad[3, 1]
    bad[5, 2] = dw.stride(0) + 1
    rc, out, out_len = _gather_raw(dw, bad, total, total, 1003)
    assert rc == 0
    want, want_len = vad_ref.gather(w, ref, 1003)
    for s in (1, 3, 5):
        want[s] = 0.0
        want_len[s] = 0
    assert np.array_equal(out[:, :1003], want) and np.array_equal(out_len, want_len)
    with pytest.raises(_native.SirError, match="sir_vad_gather"):
        ops.check_status()
    ops.check_status()                                                      # the word was cleared


def test_two_runs_are_bit_identical():
    w, dw, dl, energies, flags = _case(0.5, np.float32)
    a = _segment_raw(dw, dl, _cfg(), 4096, want_energy=True)
    b = _segment_raw(dw, dl, _cfg(), 4096, want_energy=True)
    assert a[3] == b[3] and a[3] > 0
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[4].view(np.uint32), b[4].view(np.uint32))
    ga = _gather_raw(dw, a[1][:a[3]], a[3], a[3], 4096)
    gb = _gather_raw(dw, a[1][:a[3]], a[3], a[3], 4096)
    assert np.array_equal(ga[1].view(np.uint32), gb[1].view(np.uint32)) and np.array_equal(ga[2], gb[2])


def test_segmenter_on_a_side_stream_equals_the_default_stream():
    """``Segmenter`` keeps its scratch per calling stream: ``segment`` / ``gather`` on a side stream and on the default stream give
    the same tables and clips, from two buffers."""
    w, dw, dl, _, _ = _case(0.2, np.int16)
    seg = Segmenter(chunk_size=CH, threshold=THR, silence_limit=2 * CH / 16000, prior_recording=CH / 16000)
    assert (seg.silence_chunks, seg.prior_chunks) == (2, 1)

    def run():
        table, count, total = seg.segment(dw, dl)
        return (table, count, total) + seg.gather(dw, table, total, 1003)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = run()
    side.synchronize()
    b = run()
    torch.cuda.synchronize()
    assert a[0].shape[0] > len(LENGTHS) and len(a) == 5
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ops.check_status()
    bufs = list(seg._scratch.buffers.values())
    assert len(bufs) == 2 and bufs[0].data_ptr() != bufs[1].data_ptr()


def test_bad_arguments():
    lib = _native.lib()
    h = get_featurizer().handle
    w, dw, dl, _, _ = _case(0.2, np.int16)
    EINVAL, ENOMEM = -1, -2
    for cfg in (_cfg(c=100), _cfg(c=32), _cfg(c=8192), _cfg(thr=float("nan")), _cfg(thr=-0.5), _cfg(n_stop=-1), _cfg(prior=-1)):
        assert _segment_raw(dw, dl, cfg, 16)[0] == EINVAL
    assert _segment_raw(dw, dl, _cfg(), 16, ws_bytes=64)[0] == ENOMEM
    assert lib.sir_vad_workspace_bytes(h, 4, 4096, 100) == 0
    table = torch.zeros((16, 3), dtype=torch.int32, device=DEV)
    cnt = torch.zeros((dw.shape[0],), dtype=torch.int32, device=DEV)
    tot = torch.zeros((1,), dtype=torch.int32, device=DEV)
    need = lib.sir_vad_workspace_bytes(h, dw.shape[0], dw.shape[1], CH)
    ws = torch.zeros((need,), dtype=torch.uint8, device=DEV)
    cfg = _cfg()
    good = [h, dw.data_ptr(), _native.WAVE_I16, dw.stride(0), dl.data_ptr(), dw.shape[0], dw.shape[1], C.byref(cfg), None,
            cnt.data_ptr(), table.data_ptr(), 16, tot.data_ptr(), ws.data_ptr(), need, _native.current_stream_ptr()]
    assert lib.sir_vad_segment(*good) == 0
    for i in (0, 1, 4, 7, 9, 10, 12, 13):                                   # handle, wave, lengths, cfg, seg_count, table, total, ws
        args = list(good)
        args[i] = None
        assert lib.sir_vad_segment(*args) == EINVAL, i
    args = list(good)
    args[2] = 5
    assert lib.sir_vad_segment(*args) == EINVAL
    out = torch.zeros((16, 128), dtype=torch.float32, device=DEV)
    olen = torch.zeros((16,), dtype=torch.int32, device=DEV)
    good = [h, dw.data_ptr(), _native.WAVE_I16, dw.stride(0), dw.shape[0], table.data_ptr(), tot.data_ptr(), 16, out.data_ptr(), 128, 128,
            olen.data_ptr(), _native.current_stream_ptr()]
    assert lib.sir_vad_gather(*good) == 0
    for i in (0, 1, 5, 6, 8, 11):
        args = list(good)
        args[i] = None
        assert lib.sir_vad_gather(*args) == EINVAL, i
    args = list(good)
    args[10] = 129                                                          # max_clip_len above out_stride
    assert lib.sir_vad_gather(*args) == EINVAL
    torch.cuda.synchronize()
    ops.check_status()


def test_profile_ids_are_appended():
    lib = _native.lib()
    n = lib.sir_profile_kernel_count()
    names = [lib.sir_profile_kernel_name(i).decode() for i in range(n)]
    assert names[-3:] == ["vad_chunk_energy", "vad_segment", "vad_gather"]


@pytest.mark.parametrize("pad_to", [200, None], ids=["pad200", "ragged"])
def test_recognize_recordings_end_to_end(pad_to):
    """two synthetic recordings, utterances separated by silence: start / end are the reference's, and every segment's logits are
    bit-identical to cutting the same sample ranges on the host and putting them through the featurizer and the model"""
    from sir_amd.scripts.testing import IntentRecognizer
    sr = 16000
    utt = synth.synth_clips(4, 40000, seed=77).numpy()
    z = lambda chunks: np.zeros(chunks * 1024, dtype=np.float32)       # everything chunk-aligned: energies are 0 or ~0.1
    rec0 = np.concatenate([z(8), utt[0, :24 * 1024], z(24), utt[1, :32 * 1024], z(20)])
    rec1 = np.concatenate([utt[2, :16 * 1024], z(32), utt[3, :5 * 1024], z(8)])          # the last utterance is still open
    recs = [rec0, rec1]
    torch.manual_seed(5)
    model = CNNAudioGRU(5).to(DEV).eval()
    label_map = {f"intent_{i}": i for i in range(5)}
    reco = IntentRecognizer.from_model(model, label_map, DEV)
    found = reco.recognize_recordings(recs, pad_to=pad_to)
    _, ref = vad_ref.segment_batch(recs, [len(r) for r in recs], 1024, 0.01, 7, 16, True)
    assert [len(f) for f in found] == [2, 2] and len(ref) == 4
    flat = [u for f in found for u in f]
    for u, (r, a, b) in zip(flat, ref):
        assert u["start"] == a / sr and u["end"] == b / sr
    # the host path: same ranges cut with numpy, same featurizer and model calls
    longest = int((ref[:, 2] - ref[:, 1]).max())
    limit = pad_to * HOP - 1 if pad_to is not None else longest
    clips, lens = vad_ref.gather(recs, ref, min(longest, limit))
    dl = torch.from_numpy(lens).to(DEV)
    frames = (dl // HOP + 1).clamp(min=8)
    fz = get_featurizer()
    with torch.no_grad():
        if pad_to is not None:
            want = model(fz(torch.from_numpy(clips).to(DEV), dl, t_pad=pad_to))
        else:
            want = model(fz(torch.from_numpy(clips).to(DEV), dl, t_pad=int(frames.max().item())), lengths=frames)
    want = want.cpu()
    wave, wl = reco._load_group(recs)
    table, logits = reco.score_segments(wave, wl, pad_to=pad_to)
    assert np.array_equal(table.numpy(), ref)
    assert torch.equal(logits, want)
    inv = {v: k for k, v in label_map.items()}
    for u, row in zip(flat, want):
        assert u["predicted_label"] == inv[int(row.argmax())]
        assert len(u["top_predictions"]) == 3 and abs(u["confidence"] - float(torch.softmax(row, 0).max())) < 1e-6
    ops.check_status()
