"""The float64 oracle of sir_wave_reverb_mix (tests/reverb_ref.py) against properties that do not depend on it."""
import numpy as np
import pytest

import reverb_ref as ref

RNG = np.random.default_rng(11)


def test_identity_rir():
    x = RNG.standard_normal(700)
    assert np.array_equal(ref.reverb(x, [1.0]), x)
    assert np.array_equal(ref.reverb(x, None), x)
    assert ref.reverb(np.zeros(0), [1.0, 0.5]).shape == (0,)


def test_linearity():
    x1, x2, h1, h2 = RNG.standard_normal(600), RNG.standard_normal(600), RNG.standard_normal(40), RNG.standard_normal(40)
    np.testing.assert_allclose(ref.reverb(2.0 * x1 - 3.0 * x2, h1), 2.0 * ref.reverb(x1, h1) - 3.0 * ref.reverb(x2, h1), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref.reverb(x1, h1 + 0.5 * h2), ref.reverb(x1, h1) + 0.5 * ref.reverb(x1, h2), rtol=0, atol=1e-12)


@pytest.mark.parametrize("delay", [0, 1, 37, 599, 600, 900])
def test_delayed_impulse_is_a_shift(delay):
    x = RNG.standard_normal(600)
    h = np.zeros(delay + 1)
    h[delay] = 1.0
    want = np.zeros(600)
    want[delay:] = x[:max(600 - delay, 0)]
    assert np.array_equal(ref.reverb(x, h), want)


def test_direct_sum_and_dropped_tail():
    x, h = RNG.standard_normal(50), RNG.standard_normal(80)
    y = ref.reverb(x, h)
    assert y.shape == (50,)
    for n in (0, 1, 17, 49):
        assert abs(y[n] - sum(x[n - k] * h[k] for k in range(min(80, n + 1)))) < 1e-12


@pytest.mark.parametrize("snr", [-5.0, 0.0, 20.0, 3.3])
def test_achieved_snr(snr):
    x, h, v = RNG.standard_normal(5000), RNG.standard_normal(100) * 0.1, RNG.standard_normal(700) * 0.3
    out, y, g, used = ref.mix_row(x, h, v, offset=697, snr_db=snr)
    got = 10.0 * np.log10(np.mean(y * y) / np.mean((g * used) ** 2))
    assert abs(got - snr) < 1e-9
    np.testing.assert_allclose(out - y, g * used, rtol=0, atol=1e-12)


def test_wrap_around_indexing():
    v = np.arange(7, dtype=np.float64)
    assert ref.wrapped(v, 5, 10).tolist() == [5, 6, 0, 1, 2, 3, 4, 5, 6, 0]
    assert ref.wrapped(v, 0, 3).tolist() == [0, 1, 2]
    assert ref.wrapped(v, 6, 1).tolist() == [6]
    assert ref.wrapped(v, 7 + 2, 2).tolist() == [2, 3]


def test_silence_gives_zero_gain():
    v = RNG.standard_normal(64)
    out, y, g, _ = ref.mix_row(np.zeros(100), None, v, 3, 10.0)
    assert g == 0.0 and not out.any()
    out, y, g, _ = ref.mix_row(RNG.standard_normal(100), None, np.zeros(64), 3, 10.0)
    assert g == 0.0 and np.array_equal(out, y)
    assert ref.mix_row(np.zeros(0), None, v, 3, 10.0)[2] == 0.0


def test_batch_form():
    wave = RNG.standard_normal((3, 40))
    res = ref.mix_batch(wave, [40, 0, 25], [np.array([1.0, 0.5])], [0, 0, -1], [np.ones(5)], [-1, 0, 0], [0, 1, 2], [0.0, 0.0, 6.0])
    assert np.array_equal(res[0][0], ref.reverb(wave[0], [1.0, 0.5])) and res[0][2] == 0.0
    assert res[1][0].shape == (0,)
    assert np.array_equal(res[2][1], wave[2, :25]) and res[2][2] > 0.0
