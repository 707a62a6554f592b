"""CPU: the float64 pitch / tempo contract (tests/wave_perturb_ref.py) on its own, the host helpers that must agree
with the kernel (``sir_perturb_out_len`` / ``perturbed_out_len``), the reference's augmentation draw order
(``draw_batch_params_full``) and the ``pitch_speed_augment`` training draws -- no GPU needed."""
import os
import random

import numpy as np
import pytest
import torch

import wave_perturb_ref as ref
from sir_amd import _native
from sir_amd.scripts import augment as aug

SR = 16000


def _tone(n, hz=440.0):
    return 0.5 * np.sin(2 * np.pi * hz * np.arange(n) / SR)


def _peak_bin(y):
    return int(np.argmax(np.abs(np.fft.rfft(y * np.hanning(len(y))))))


def test_geometry_at_16k():
    assert ref.geometry(16000) == (1312, 235, 192, 1120)


@pytest.mark.parametrize("f", [0.85, 0.9, 1.1, 1.15])
def test_tempo_keeps_pitch_and_sets_length(f):
    x = _tone(24000)
    y, offs, costs = ref.tempo(x, f)
    n = int(24000 / f + 0.5)
    assert len(y) == n and len(offs) == -(-n // 1120) and len(costs) == len(offs) - 1
    assert abs(_peak_bin(y) - 440.0 * n / SR) <= 1.0
    # segments after the first pick the offset whose overlap matches the running output best
    assert all(c[o] == c.min() for c, o in zip(costs, offs[1:]))


@pytest.mark.parametrize("c", [-200.0, -37.5, 150.0, 200.0])
def test_pitch_moves_the_peak_and_keeps_length(c):
    x = _tone(24000)
    y, offs, costs, s = ref.pitch(x, c)
    d = 2.0 ** (c / 1200.0)
    assert len(y) == 24000 and len(s) == int(24000 * d + 0.5)
    assert abs(_peak_bin(y) - 440.0 * d * 24000 / SR) <= 1.0


def test_identity_and_short_clips():
    x = np.random.default_rng(0).standard_normal(5000)
    assert np.array_equal(ref.tempo(x, 1.0)[0], x) and np.array_equal(ref.pitch(x, 0.0)[0], x)
    for n in (0, 1, 300, 1312):
        for f in (0.85, 1.15):
            y, offs, _ = ref.tempo(x[:n], f)
            assert len(y) == int(n / f + 0.5) and len(offs) == -(-len(y) // 1120)
        assert len(ref.pitch(x[:n], 150.0)[0]) == n
    # a clip shorter than one hop is its first samples, zero-extended (segment 0 is z[W/2 ..] = x)
    y, _, _ = ref.tempo(x[:300], 0.85)
    assert np.array_equal(y[:300], x[:300]) and (y[300:] == 0).all()


def test_shift_matches_feature_kernel_convention():
    x = np.arange(1.0, 11.0)
    assert ref.shifted(x, 3).tolist() == [0, 0, 0, 1, 2, 3, 4, 5, 6, 7]
    assert ref.shifted(x, -2).tolist() == [3, 4, 5, 6, 7, 8, 9, 10, 0, 0]
    assert (ref.shifted(x, 20) == 0).all() and (ref.shifted(x, -20) == 0).all()


def _lib():
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.lib()


def test_out_len_host_helpers_agree():
    lib = _lib()
    rng = np.random.default_rng(5)
    factors = [0.5, 0.85, 0.9, 1.0, 1.1, 1.15, 2.0] + rng.uniform(0.85, 1.15, 200).tolist()
    for L in [0, 1, 299, 300, 1312, 5000, 47999, 48000, 80000]:
        for f in factors:
            f32 = float(np.float32(f))
            want = lib.sir_perturb_out_len(L, f32)
            assert aug.perturbed_out_len(L, f) == want == ref.out_len(L, f32), (L, f)
    assert lib.sir_perturb_out_len(-1, 1.0) == -1 and lib.sir_perturb_out_len(10, 0.0) == -1


def _reference_draws(lengths, p, rng):
    """What augment.py:98-135 draws from `random`, clip by clip (its effects replaced by the draws they make)."""
    out = []
    for n in lengths:
        s, c, t, g = 0, 0.0, 1.0, 0.0
        if rng.random() < p:
            if rng.random() < 0.5:
                s = int(rng.uniform(-0.1, 0.1) * n)                 # time_shift, augment.py:18
            if rng.random() < 0.5:
                c = float(rng.uniform(-2.0, 2.0)) * 100             # pitch_shift, :43 + :47
            if rng.random() < 0.5:
                t = float(rng.uniform(0.85, 1.15))                  # speed_change, :68
            if rng.random() < 0.5:
                g = float(rng.uniform(0.001, 0.01))                 # add_noise, :93
        out.append((s, c, t, g))
    return out


def test_draw_batch_params_full_replays_reference_sequence():
    lengths = [48000, 30000, 16000, 700] * 100
    shift, cents, tempo, sigma = aug.draw_batch_params_full(lengths, 0.7, random.Random(11))
    want = _reference_draws(lengths, 0.7, random.Random(11))
    assert shift.dtype == torch.int32 and cents.dtype == tempo.dtype == sigma.dtype == torch.float32
    assert shift.tolist() == [w[0] for w in want]
    assert np.array_equal(cents.numpy(), np.float32([w[1] for w in want]))
    assert np.array_equal(tempo.numpy(), np.float32([w[2] for w in want]))
    assert np.array_equal(sigma.numpy(), np.float32([w[3] for w in want]))
    # marginal rates of the gating: 0.7 * 0.5 each
    n = len(lengths)
    for drawn in (cents != 0, tempo != 1, sigma > 0):
        assert 0.27 < drawn.float().mean().item() < 0.43
    assert (cents.abs() <= 200).all() and ((tempo >= 0.85) & (tempo <= 1.15)).all()
    s0, c0, t0, g0 = aug.draw_batch_params_full([48000] * 50, 0.0, random.Random(1))
    assert (s0 == 0).all() and (c0 == 0).all() and (t0 == 1).all() and (g0 == 0).all() and n == 400


def test_make_waveform_augment_pitch_speed_keys_and_masks():
    from sir_amd.scripts import train as tr
    lengths = [48000, 30000, 16000, 700, 0, 47999]
    cfg = {"fused_features": True, "pitch_speed_augment": True, "augment_prob": 1.0, "waveform_augment_prob": 1.0}
    fn = tr.make_waveform_augment(cfg, seed=4, epoch=2)
    seen_tempo = False
    for idx in range(20):
        kw = fn(idx, len(lengths), lengths)
        assert set(kw) == {"shift", "pitch_cents", "tempo", "noise_sigma", "noise_seed", "time_mask", "freq_mask"}
        frames = [1 + aug.perturbed_out_len(n, f) // 512 for n, f in zip(lengths, kw["tempo"].tolist())]
        tm = kw["time_mask"]
        assert all(int(tm[b, 0]) + int(tm[b, 1]) <= max(frames[b], int(tm[b, 1])) for b in range(len(lengths)))
        seen_tempo |= bool((kw["tempo"] != 1).any())
    assert seen_tempo
    # the draws replay draw_batch_params_full then draw_spec_masks on one stream, masks against the perturbed frames
    rng = random.Random((4 << 20) ^ 2)
    shift, cents, tempo, sigma = aug.draw_batch_params_full(lengths, 1.0, rng)
    tm, fm = aug.draw_spec_masks([1 + aug.perturbed_out_len(n, f) // 512 for n, f in zip(lengths, tempo.tolist())], 1.0,
                                 rng=rng)
    kw = tr.make_waveform_augment(cfg, seed=4, epoch=2)(0, len(lengths), lengths)
    assert torch.equal(kw["tempo"], tempo) and torch.equal(kw["pitch_cents"], cents) and torch.equal(kw["time_mask"], tm)


def test_make_waveform_augment_unchanged_without_the_key():
    from sir_amd.scripts import train as tr
    lengths = [48000, 30000, 16000, 700]
    cfg = {"fused_features": True, "waveform_augment": True, "augment_prob": 0.7}
    kw = tr.make_waveform_augment(cfg, seed=1, epoch=0)(0, 4, lengths)
    assert set(kw) == {"shift", "noise_sigma", "noise_seed", "time_mask", "freq_mask"}
    rng = random.Random(1 << 20)
    shift, sigma = aug.draw_batch_params(lengths, 0.7, rng)
    tm, fm = aug.draw_spec_masks([1 + n // 512 for n in lengths], 0.7, rng=rng)
    assert torch.equal(kw["shift"], shift) and torch.equal(kw["noise_sigma"], sigma)
    assert torch.equal(kw["time_mask"], tm) and torch.equal(kw["freq_mask"], fm)
    kw_off = tr.make_waveform_augment(dict(cfg, pitch_speed_augment=False), seed=1, epoch=0)(0, 4, lengths)
    assert all(torch.equal(kw_off[k], kw[k]) for k in ("shift", "noise_sigma", "time_mask", "freq_mask"))
