"""CPU: the ring cases of tests/reverb_cases.py tell a correct spectrum ring from a broken one.

reverb_ref.ols_ring_model restates the kernel's schedule in float32.  With the kernel's ring of parts + 3 slots it stays within
the kernel's own bound, 1e-5 |x|_inf |h|_1, of the float64 oracle on every row of every case; with a ring one slot short (a
round's fourth spectrum then lands on the oldest one still to be read) it misses that bound by at least 10x on EVERY row whose
RIR fills the ring (P = parts), and so does dropping a RIR's last partition on every row with P >= 2.  No case and no row is
left out: a case that passed here with a broken ring would prove nothing on the GPU."""
import numpy as np
import pytest

import reverb_cases as rc
import reverb_ref as ref

BOUND = 1e-5


def _ratio(y, want, bound):
    return np.abs(y.astype(np.float64) - want).max() / bound


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_cases_tell_a_correct_ring_from_a_broken_one(case):
    c, want = rc.ring_case(*case), rc.oracle(*case)
    parts = c["parts"]
    assert c["max_len"] == 512 * (2 * c["ring"] + 5) and max(n for _, _, n in c["rows"]) == c["max_len"]
    assert {-(-n // 512) % 4 for _, r, n in c["rows"] if r >= 0} == {0, 1, 2, 3}              # last rounds of 1, 2, 3 and 4 blocks
    full = with_parts = 0
    for b, (_, r, n) in enumerate(c["rows"]):
        if r < 0:
            continue
        x, h = c["x64"][b, :n].astype(np.float32), c["rirs"][r]
        y64, bound = want[b]
        p = -(-len(h) // 512)
        assert p <= parts and len(h) <= c["max_rir_len"]
        good = _ratio(ref.ols_ring_model(x, h, parts), y64, bound)
        assert good <= BOUND, (b, c["names"][r], good)
        if p == parts:
            short = _ratio(ref.ols_ring_model(x, h, parts, ring_extra=2), y64, bound)
            assert short >= 10 * BOUND, (b, c["names"][r], short)
            full += 1
        else:                                                     # P < parts leaves a slot to spare: the short ring still works
            assert _ratio(ref.ols_ring_model(x, h, parts, ring_extra=2), y64, bound) <= BOUND
        if p >= 2:
            lost = _ratio(ref.ols_ring_model(x, h[:512 * (p - 1)], parts), y64, bound)
            assert lost >= 10 * BOUND, (b, c["names"][r], lost)
            with_parts += 1
    assert full >= 5 and (with_parts >= 5 or parts == 1)


def test_the_model_follows_its_arguments():
    """ring_extra >= 3 and the number of waves do not change what a correct ring computes; one wave needs no extra slot"""
    gen = np.random.default_rng(3)
    x, h = gen.standard_normal(7000).astype(np.float32), gen.standard_normal(1500).astype(np.float32)
    want = ref.reverb(x, h)
    bound = np.abs(x).max() * np.abs(h).sum()
    base = ref.ols_ring_model(x, h, 3)
    assert _ratio(base, want, bound) <= BOUND
    assert np.array_equal(ref.ols_ring_model(x, h, 5, ring_extra=7), base)
    assert np.array_equal(ref.ols_ring_model(x, h, 3, ring_extra=0, waves=1), base)
    assert _ratio(ref.ols_ring_model(x, h, 3, ring_extra=0, waves=2), want, bound) > 10 * BOUND


def test_noise_gain_is_total():
    y, v = np.full(10, 0.5), np.full(10, 0.25)
    assert ref.noise_gain(y, v, 0.0) == (2.0, True)
    assert ref.noise_gain(y, v, 3e38) == (0.0, True) and ref.noise_gain(y, v, 400.0)[1]
    g, finite = ref.noise_gain(y, v, -3e38)
    assert g == float("inf") and not finite
    g, finite = ref.noise_gain(y, v, -1000.0)
    assert np.isfinite(g) and not finite                          # 2e50: a float64, no float32
    g, finite = ref.noise_gain(y, v, -300.0)
    assert finite and abs(g - 2e15) <= 1e-9 * 2e15
    assert not ref.noise_gain(y, v, float("nan"))[1]
    out, _, g, _ = ref.mix_row(y, None, v, 0, -1000.0)            # a bad row: zeroed, gain 0
    assert g == 0.0 and not out.any()
    out, _, g, _ = ref.mix_row(y, None, v, 0, 3e38)
    assert g == 0.0 and np.array_equal(out, y)
