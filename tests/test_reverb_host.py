"""Host side of the reverb / background-noise stage: the ABI table, the draws, the banks, the rejected differentiable forms."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from sir_amd import _native, synth
from sir_amd.scripts import augment as aug
from sir_amd.scripts import train as tr
from sir_amd.sound_bank import MAX_RIR_TAPS, SoundBank, prepare_rir

SYMBOLS = ("sir_reverb_workspace_bytes", "sir_wave_reverb_mix")
LENGTHS = [[48000, 16000, 30000, 700], [512, 48000, 20000, 33333], [1000, 2000, 3000, 4000], [48000] * 4, [9, 99, 999, 9999]]


def test_symbols_in_signatures_and_library():
    for name in SYMBOLS:
        assert name in _native.SIGNATURES
    assert len(_native.SIGNATURES["sir_wave_reverb_mix"][1]) == 25
    assert os.path.exists(_native.LIB_PATH), "libsir_hip.so has not been built (python __graft_entry__.py)"
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.sir_abi_version() == 1


def _five_batches(cfg, seed=5):
    fn = tr.make_waveform_augment(cfg, seed=seed, epoch=3)
    return [fn(i, len(n), n) for i, n in enumerate(LENGTHS)]


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    return a == b


@pytest.mark.parametrize("base", [{}, {"waveform_augment": True}, {"pitch_speed_augment": True, "augment_prob": 0.9}])
def test_existing_keys_unchanged_when_off(base):
    want = _five_batches(dict(base))
    absent_false = _five_batches(dict(base, reverb_augment=False, background_noise_augment=False))
    prob0 = _five_batches(dict(base, reverb_augment=True, reverb_prob=0.0, background_noise_augment=True, noise_prob=0.0))
    for w, a, p in zip(want, absent_false, prob0):
        assert set(a) == set(w)                                   # the dictionary itself is what it was
        for k in w:
            assert _same(w[k], a[k]), k
            assert _same(w[k], p[k]), k
        assert not (set(p) - set(w)) & {"rir_index", "noise_index"}   # probability 0 draws nothing and adds nothing


def test_new_draws_come_last_and_stay_in_range():
    base = {"pitch_speed_augment": True}
    want = _five_batches(dict(base))[0]
    cfg = dict(base, reverb_augment=True, reverb_prob=0.6, rt60_range=(0.1, 0.3), background_noise_augment=True, noise_prob=0.7,
               snr_db_range=(3.0, 12.0))
    got = _five_batches(cfg)
    for k in want:                                                # first batch: every existing draw precedes the new ones
        assert _same(want[k], got[0][k]), k
    seen_r = seen_n = seen_off = 0
    for kw, n in zip(got, LENGTHS):
        rir, noise = kw["rir"], kw["noise"]
        assert rir.kind == "rir" and len(rir) == 32 and noise.kind == "noise" and len(noise) == 8
        ri, ni, off, snr = (kw[k] for k in ("rir_index", "noise_index", "noise_offset", "snr_db"))
        assert ri.dtype == ni.dtype == off.dtype == torch.int32 and snr.dtype == torch.float32
        assert ri.shape == ni.shape == off.shape == snr.shape == (len(n),)
        assert int(ri.min()) >= -1 and int(ri.max()) < len(rir) and int(ni.min()) >= -1 and int(ni.max()) < len(noise)
        for b in range(len(n)):
            if int(ni[b]) >= 0:
                assert 0 <= int(off[b]) < noise.host_lengths[int(ni[b])]
                assert 3.0 <= float(snr[b]) <= 12.0
                seen_off += int(off[b]) > 0
        seen_r += int((ri >= 0).sum())
        seen_n += int((ni >= 0).sum())
    assert 0 < seen_r < 20 and 0 < seen_n < 20 and seen_off > 0


def test_draw_function_alone():
    rng = random.Random(1)
    out = aug.draw_reverb_noise_params([100] * 64, {"n_rir": 3, "reverb_prob": 1.0}, rng)
    assert set(out) == {"rir_index"} and set(out["rir_index"].tolist()) == {0, 1, 2}
    out = aug.draw_reverb_noise_params([100] * 64, {"noise_lengths": [5, 1], "noise_prob": 1.0, "snr_db_range": (0.0, 0.0)}, rng)
    assert set(out) == {"noise_index", "noise_offset", "snr_db"}
    assert all(0 <= o < (5, 1)[v] for o, v in zip(out["noise_offset"].tolist(), out["noise_index"].tolist()))
    state = rng.getstate()
    assert aug.draw_reverb_noise_params([100] * 4, {"n_rir": 3, "reverb_prob": 0.0, "noise_lengths": [5], "noise_prob": 0.0}, rng) == {}
    assert rng.getstate() == state


def test_prepare_rir_alignment_cut_and_scale():
    h = torch.zeros(10000)
    h[40], h[41], h[300], h[9000] = -0.5, 0.25, 0.5, 0.1          # two taps of the peak magnitude: the first is the direct path
    p = prepare_rir(h)
    assert p.dtype == torch.float32 and p.numel() == MAX_RIR_TAPS
    assert float(p[0]) == -1.0 and float(p[1]) == 0.5 and float(p[260]) == 1.0 and float(p.abs().max()) == 1.0
    assert float(p[8191]) == 0.0 and not p[8000:].any()          # tap 9000 - 40 = 8960 lies behind the cut
    assert prepare_rir([0.0, 0.0, 4.0]).tolist() == [1.0]
    for bad in ([], [0.0, 0.0], [1.0, float("nan")]):
        with pytest.raises(ValueError):
            prepare_rir(bad)


def test_sound_bank_layout():
    gen = np.random.default_rng(3)
    clips = [synth.synthetic_rir(0.05, rng=gen), torch.tensor([0.0, 0.0, -2.0, 1.0]), synth.synthetic_rir(2.0, rng=gen)]
    bank = SoundBank(clips, kind="rir")
    assert len(bank) == 3 and bank.host_lengths == [800, 2, 8192] and bank.max_len == 8192
    assert bank.data.dtype == torch.float32 and bank.data.shape[0] == 3 and bank.data.shape[1] % 8 == 0 and bank.data.shape[1] >= 8192
    assert bank.lengths.dtype == torch.int32 and bank.lengths.tolist() == bank.host_lengths
    assert bank.data[1, :4].tolist() == [-1.0, 0.5, 0.0, 0.0]
    for i, n in enumerate(bank.host_lengths):
        assert float(bank.data[i, :n].abs().max()) == 1.0 and abs(float(bank.data[i, 0])) == 1.0 and not bank.data[i, n:].any()
    noise = SoundBank([synth.coloured_noise(1000, gen), synth.coloured_noise(333, gen, exponent=2.0)])
    assert noise.kind == "noise" and noise.host_lengths == [1000, 333] and noise.on("cpu") is noise
    assert abs(float(noise.data[0, :1000].square().mean().sqrt()) - 0.05) < 1e-6
    with pytest.raises(ValueError):
        SoundBank([])
    with pytest.raises(ValueError):
        SoundBank([torch.zeros(0)])


def test_sound_bank_from_dir(tmp_path):
    from sir_amd.scripts.utils import wav_io
    gen = np.random.default_rng(4)
    a, b = synth.coloured_noise(4000, gen) * 4.0, synth.coloured_noise(2500, gen) * 4.0
    wav_io.write_wav_pcm16(str(tmp_path / "b.wav"), a, 16000)
    os.makedirs(tmp_path / "sub")
    wav_io.write_wav_pcm16(str(tmp_path / "sub" / "a.wav"), torch.stack([b, b]), 16000)     # stereo: mixed down
    (tmp_path / "notes.txt").write_text("not audio")
    bank = SoundBank.from_dir(str(tmp_path), max_seconds=0.2)
    assert bank.host_lengths == [3200, 2500]
    assert torch.allclose(bank.data[0, :3200], a[:3200], atol=1.0 / 32768) and torch.allclose(bank.data[1, :2500], b, atol=1.0 / 32768)
    with pytest.raises(ValueError):
        SoundBank.from_dir(str(tmp_path / "sub" / "none"))


def test_synthetic_generators():
    gen = np.random.default_rng(0)
    h = synth.synthetic_rir(0.3, rng=gen)
    assert h.dtype == torch.float32 and h.numel() == 4800 and float(h[0]) == 1.0 and float(h[1:].abs().max()) < 1.0
    early, late = h[1:801].square().mean().sqrt(), h[4000:].square().mean().sqrt()
    assert 20.0 * np.log10(float(early / late)) > 30.0            # the envelope falls by 60 dB over the response
    assert torch.equal(synth.synthetic_rir(0.3, rng=np.random.default_rng(0)), h)
    assert synth.synthetic_rir(5.0, rng=gen).numel() == 8192
    with pytest.raises(ValueError):
        synth.synthetic_rir(0.0)
    x = synth.coloured_noise(16000, gen, exponent=2.0)
    spec = np.abs(np.fft.rfft(x.numpy())) ** 2
    assert spec[1:200].mean() > 100.0 * spec[4000:].mean()


def test_differentiable_forms_reject_the_new_arguments():
    from sir_amd import explain
    from sir_amd.featurizer import HipFeaturizer
    fz = HipFeaturizer.__new__(HipFeaturizer)                     # no device call is reached
    wave = torch.zeros(2, 4000)
    idx = torch.zeros(2, dtype=torch.int32)
    for kw in ({"rir_index": idx}, {"noise_index": idx, "noise_offset": idx, "snr_db": torch.zeros(2)}, {"rir": object()}):
        with pytest.raises(ValueError, match="reverb"):
            fz.differentiable(wave, t_pad=24, **kw)
        with pytest.raises(ValueError, match="reverb"):
            explain.wave_gradient(None, wave, t_pad=24, **kw)
        with pytest.raises(ValueError, match="reverb"):
            explain.fgsm_wave(None, wave, idx, 0.01, t_pad=24, **kw)
    with pytest.raises(TypeError):
        fz.differentiable(wave, t_pad=24, no_such_argument=1)
