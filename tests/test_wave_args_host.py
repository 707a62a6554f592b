"""CPU: the one argument path of the waveform wrappers (``sir_amd/wave_args.py``).  The batch check and the ``out`` check against
tables of malformed inputs, every wrapper through that path with each library call barred, and the per-stream scratch cache
with host stand-ins for the device.  No device call is made."""
import types

import pytest
import torch

from sir_amd import _native, wave_args
from sir_amd.featurizer import HipFeaturizer
from sir_amd.segmenter import Segmenter

B, L = 3, 40


def _bar_device(monkeypatch):
    """tests/test_adversarial_host.py's pattern, with the device check accepting host tensors: what raises below raises from
    the metadata checks, ahead of any library call."""
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_native, "lib", no_device)
    monkeypatch.setattr(_native, "current_stream_ptr", no_device)
    monkeypatch.setattr(_native, "require_hip", lambda *tensors: None)


def _wave(dtype=torch.float32, rows=B):
    return torch.zeros(rows, L, dtype=dtype)


MALFORMED = {
    "rank 1": (torch.zeros(L), None),
    "rank 3": (torch.zeros(B, 1, L), None),
    "inner stride 2": (torch.zeros(B, 2 * L)[:, ::2], None),
    "int32": (_wave(torch.int32), None),
    "float64": (_wave(torch.float64), None),
    "float lengths": (_wave(), torch.full((B,), float(L))),
    "bool lengths": (_wave(), torch.ones(B, dtype=torch.bool)),
    "2-D lengths": (_wave(), torch.full((B, 1), L, dtype=torch.int32)),
    "B - 1 lengths": (_wave(), torch.full((B - 1,), L, dtype=torch.int32)),
    "B + 1 lengths": (_wave(), torch.full((B + 1,), L, dtype=torch.int32)),
}


@pytest.mark.parametrize("case", list(MALFORMED))
def test_batch_check_refuses(case, monkeypatch):
    _bar_device(monkeypatch)
    wave, lengths = MALFORMED[case]
    assert wave.stride(-1) == (2 if case == "inner stride 2" else 1)
    with pytest.raises(_native.SirError, match="some_caller"):
        wave_args.check_batch("some_caller", wave, lengths)


def test_batch_check_refuses_an_empty_batch_where_asked(monkeypatch):
    _bar_device(monkeypatch)
    for empty in (torch.zeros(0, L), torch.zeros(B, 0)):
        with pytest.raises(_native.SirError, match="some_caller needs a non-empty"):
            wave_args.check_batch("some_caller", empty, refuse_empty=True)
        code, rows, max_len, lengths = wave_args.check_batch("some_caller", empty)
        assert (code, rows, max_len) == (_native.WAVE_F32,) + tuple(empty.shape) and lengths.shape == (empty.shape[0],)


@pytest.mark.parametrize("dtype,code", [(torch.float32, _native.WAVE_F32), (torch.int16, _native.WAVE_I16)])
def test_batch_check_accepts(dtype, code, monkeypatch):
    _bar_device(monkeypatch)
    strided = torch.zeros(B, L + 24, dtype=dtype)[:, :L]                 # a row stride above L
    assert strided.stride() == (L + 24, 1)
    for wave in (_wave(dtype), strided):
        got = wave_args.check_batch("some_caller", wave)
        assert got[:3] == (code, B, L)
        assert got[3].dtype == torch.int32 and got[3].device == wave.device and got[3].tolist() == [L] * B
        given = torch.tensor([L, 9, 0, 9, 7, 9], dtype=torch.int64)[::2]                      # int64, not contiguous
        assert not given.is_contiguous()
        got = wave_args.check_batch("some_caller", wave, given, refuse_empty=True)
        assert got[:3] == (code, B, L)
        assert got[3].dtype == torch.int32 and got[3].is_contiguous() and got[3].tolist() == [L, 0, 7]


def test_batch_check_of_a_stream_push(monkeypatch):
    """a fixed row count and the stream's one dtype, in one message as ``StreamInput.push`` words it"""
    _bar_device(monkeypatch)
    kw = dict(must="samples must be torch.uint8 [3, <= 64]", rows=B, dtypes={torch.uint8: _native.WAVE_ULAW})
    code, rows, width, lengths = wave_args.check_batch("push", _wave(torch.uint8), None, "stream", **kw)
    assert (code, rows, width, lengths.tolist()) == (_native.WAVE_ULAW, B, L, [L] * B)
    for bad in (_wave(torch.int16), _wave(torch.uint8, rows=B + 1), torch.zeros(L, dtype=torch.uint8)):
        with pytest.raises(_native.SirError, match=r"push: samples must be torch.uint8 \[3, <= 64\] with unit inner stride"):
            wave_args.check_batch("push", bad, None, "stream", **kw)
    with pytest.raises(_native.SirError, match="push: lengths must hold one entry per stream: 2 for 3"):
        wave_args.check_batch("push", _wave(torch.uint8), torch.zeros(B - 1, dtype=torch.int32), "stream", **kw)


def test_the_device_check_comes_first():
    """unpatched, host tensors stop at ``require_hip`` (with or without a GPU in the machine)"""
    with pytest.raises(_native.SirError, match="HIP device"):
        wave_args.check_batch("some_caller", _wave())


def test_out_check(monkeypatch):
    _bar_device(monkeypatch)
    cpu = torch.device("cpu")
    new = wave_args.check_out(None, B, L, cpu)
    assert new.shape == (B, L) and new.dtype == torch.float32
    wide = torch.zeros(B, L + 8)
    assert wave_args.check_out(wide, B, L, cpu) is wide and wave_args.check_out(wide[:, :L], B, L, cpu).stride(0) == L + 8
    assert wave_args.first_cols(wide, L).shape == (B, L) and wave_args.first_cols(wide, L + 8) is wide
    bad = {"dtype": torch.zeros(B, L, dtype=torch.float64), "rows": torch.zeros(B + 1, L), "narrow": torch.zeros(B, L - 1),
           "inner stride 2": torch.zeros(B, 2 * L)[:, ::2], "rank": torch.zeros(B * L)}
    for name, out in bad.items():
        with pytest.raises(_native.SirError, match=r"out must be float32 \[B, >= L\] with unit inner stride"):
            wave_args.check_out(out, B, L, cpu)
    with pytest.raises(_native.SirError, match=r"out must be float32 \[3, >= 40\]"):
        wave_args.check_out(bad["narrow"], B, L, cpu, "[3, >= 40]")
    # the row stride handed to the library: as it is for several rows, at least the width for a single one
    assert wave_args.out_row_stride(wide[:, :L]) == L + 8
    one = torch.zeros(1, L + 8)
    assert wave_args.out_row_stride(one) == L + 8
    assert wave_args.out_row_stride(torch.as_strided(one, (1, L + 8), (1, 1))) == L + 8
    assert wave_args.out_row_stride(torch.as_strided(torch.zeros(4 * L), (1, L), (3 * L, 1))) == 3 * L


def test_keep_holds_and_counts(monkeypatch):
    _bar_device(monkeypatch)
    keep = wave_args.Keep(torch.device("cpu"), rows=B)
    assert keep.ptr(None, torch.int32) is None and keep.held == []
    p = keep.ptr([1, 2, 3], torch.int32)
    assert p == keep.held[0].data_ptr() and keep.held[0].dtype == torch.int32
    with pytest.raises(_native.SirError, match="per-utterance argument of 2 values for a batch of 3"):
        keep.ptr(torch.zeros(2), torch.float32)
    free = wave_args.Keep(torch.device("cpu"))
    assert free.augment(None, None, 0, None, None) is None and free.held == []
    assert free.augment(torch.zeros(5), None, 7, None, None) is not None and len(free.held) == 1


def _featurizer():
    fz = object.__new__(HipFeaturizer)                                   # (no handle: creating one is a device call)
    fz.sample_rate, fz.n_mels, fz.n_fft, fz.hop_length, fz.win_length, fz._h = 16000, 64, 1024, 512, 1024, None
    return fz


def _wrappers():
    fz = _featurizer()
    grads = torch.zeros(B, 64, 8)
    return {
        "features": lambda wave, lengths: fz(wave, lengths, t_pad=8),
        "features_bwd": lambda wave, lengths: fz.features_bwd(wave, lengths, grads, grads, t_pad=8),
        "resample": lambda wave, lengths: fz.resample(wave, 8000, 16000, lengths),
        "perturb": lambda wave, lengths: fz.perturb(wave, lengths, tempo=torch.ones(B)),
        "reverb_mix": lambda wave, lengths: fz.reverb_mix(wave, lengths),
    }


@pytest.mark.parametrize("who", ["features", "features_bwd", "resample", "perturb", "reverb_mix", "Segmenter.segment"])
def test_every_wrapper_checks_ahead_of_the_library(who, monkeypatch):
    _bar_device(monkeypatch)
    # (no Segmenter constructor: it asks the library for its host arithmetic, and segment() reads nothing of it this far)
    call = object.__new__(Segmenter).segment if who == "Segmenter.segment" else _wrappers()[who]
    with pytest.raises(_native.SirError, match=f"{who}: lengths must hold one entry per"):
        call(_wave(), torch.full((B - 1,), L, dtype=torch.int32))
    with pytest.raises(_native.SirError, match=f"{who}: unsupported waveform dtype torch.int32"):
        call(_wave(torch.int32), None)
    with pytest.raises(AssertionError, match="a device call was made"):  # a good batch goes on to the library
        call(_wave(), torch.full((B,), L, dtype=torch.int32))


def test_features_bwd_refuses_a_narrow_out(monkeypatch):
    _bar_device(monkeypatch)
    grads = torch.zeros(B, 64, 8)
    with pytest.raises(_native.SirError, match="out must be float32"):
        _featurizer().features_bwd(_wave(), None, grads, grads, t_pad=8, out=torch.zeros(B, L - 1))


def test_scratch_is_kept_per_stream_and_only_grows(monkeypatch):
    current = types.SimpleNamespace(cuda_stream=11)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: current)
    cpu = torch.device("cpu")
    scratch = wave_args.StreamScratch()
    a = scratch.get(1000, cpu)
    assert a.dtype == torch.uint8 and a.numel() == 1000
    assert scratch.get(1000, cpu) is a and scratch.get(10, cpu) is a     # the same key: the same buffer
    current.cuda_stream = 12
    b = scratch.get(0, cpu)                                              # another stream: a buffer of its own, never empty
    assert b is not a and b.numel() == wave_args.StreamScratch.MIN_BYTES == 256
    assert b.data_ptr() != a.data_ptr() and scratch.get(256, cpu) is b
    grown = scratch.get(5000, cpu)                                       # a larger request replaces this key's buffer only
    assert grown is not b and grown.numel() == 5000 and scratch.get(300, cpu) is grown
    current.cuda_stream = 11
    assert scratch.get(1000, cpu) is a
    assert set(scratch.buffers) == {(cpu, 11), (cpu, 12)}
