"""CPU: the conditions the GPU comparisons of tests/test_frontend_edge_gpu.py rest on -- the float64 filter of
tests/frontend_edge_ref.py against the oracle's float32 taps, the oracle itself inside the bound the kernel is held to, the
impulse batches reaching every tap, the decode margin of ``AudioFeatureExtractor._load`` covering the filter's support -- and
the host helper ``sir_resample_out_len``.

``HipFeaturizer.resample`` raises ``SirError`` where the helper answers -1; reaching that needs a clip of several gigabytes
on the device, so it has no test of its own."""
import numpy as np
import pytest
import torch

import frontend_edge_ref as ref
from oracle import resample_ref
from sir_amd import _native

INT_MAX = 2 ** 31 - 1


def _ulps32(a64, b32):
    """|a - b| in units of b's float32 spacing (b32 float32, a64 float64)."""
    b = b32.astype(np.float64)
    return np.abs(a64 - b) / np.maximum(np.spacing(np.abs(b32)).astype(np.float64), 2.0 ** -149)


@pytest.mark.parametrize("orig_freq,new_freq", ref.PAIRS)
def test_float64_taps_round_to_the_oracles(orig_freq, new_freq):
    orig, nw = ref.reduced(orig_freq, new_freq)
    w = ref.width(orig_freq, new_freq)
    kernel, kw = resample_ref.sinc_resample_kernel(orig_freq, new_freq)
    kernel = kernel[:, 0].numpy()
    assert kw == w and kernel.shape == (nw, 2 * w + orig)
    d, h = ref.taps64(orig_freq, new_freq)
    mine = (d >= -w) & (d < w + orig)                                  # the offsets the oracle's kernel spans
    assert (h[:, ~mine] == 0).all() and (~mine[:2]).all() and (~mine[-2:]).all()      # nothing outside, on both sides
    h = h[:, mine]
    h32 = h.astype(np.float32)
    not_nearest = int((h32 != kernel).sum())
    worst = float(_ulps32(h, kernel).max())
    print(f"taps {orig_freq}->{new_freq} ({orig}:{nw}): {int((h != 0).sum())} nonzero, {not_nearest} not the nearest float32, "
          f"worst {worst:.3f} ulp")
    assert worst <= 1.0
    assert ((kernel == 0) == (h == 0)).all()                           # the oracle's out-of-window taps are exactly 0.0f
    assert ((h32 == 0) == (h == 0)).all()                              # and no tap underflows on the cast


@pytest.mark.parametrize("orig_freq,new_freq", ref.RANDOM_PAIRS)
def test_oracle_stays_inside_the_bound_on_the_random_cases(orig_freq, new_freq):
    case = ref.random_case(orig_freq, new_freq)
    worst = 0.0
    for b, n in enumerate(case["used"]):
        for x in (case["f32"][b, :n].astype(np.float64), case["i16"][b, :n].astype(np.float64) / 32768.0):
            assert np.isfinite(x).all()
            y, s = ref.resample64(x, orig_freq, new_freq)
            assert len(y) == ref.out_len(n, orig_freq, new_freq) == resample_ref.output_length(n, orig_freq, new_freq)
            if n == 0:
                continue
            got = resample_ref.resample(torch.from_numpy(x.astype(np.float32))[None], orig_freq, new_freq)[0].numpy()
            bound = ref.resample_bound(s, orig_freq, new_freq)
            err = np.abs(got.astype(np.float64) - y)
            assert (err <= bound).all(), (b, n)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    assert (case["lengths"][-2:] == [case["f32"].shape[1] + 1000, -1000]).all()
    assert np.isnan(case["f32"][-1]).all() and (case["i16"][-1] == 32767).all()
    print(f"oracle {orig_freq}->{new_freq}: worst err / bound {worst:.3f} over lengths {case['used']}")


@pytest.mark.parametrize("orig_freq,new_freq", [(44100, 8000), (16000, 44100), (12000, 16000)])
def test_windowed_sum_is_the_dense_sum(orig_freq, new_freq):
    rng = np.random.Generator(np.random.PCG64(1))
    x = rng.standard_normal(2 * ref.reduced(orig_freq, new_freq)[0] + 5)
    y, s = ref.resample64(x, orig_freq, new_freq)
    yd, sd = ref.resample64_dense(x, orig_freq, new_freq)
    assert (np.abs(y - yd) <= 1e-15 * sd).all() and (np.abs(s - sd) <= 1e-15 * sd).all()
    # ... and an impulse row of it is the one-term form the impulse tests use
    length, q = ref.impulse_case(orig_freq, new_freq)
    for pos in (q[0], q[-3], q[-2], q[-1]):
        x = np.zeros(length)
        x[pos] = 0.5
        assert np.array_equal(ref.resample64(x, orig_freq, new_freq)[0], ref.impulse64(pos, 0.5, length, orig_freq, new_freq))


@pytest.mark.parametrize("orig_freq,new_freq", ref.PAIRS)
def test_impulse_rows_visit_every_tap(orig_freq, new_freq):
    orig, nw = ref.reduced(orig_freq, new_freq)
    length, q = ref.impulse_case(orig_freq, new_freq)
    assert len(q) == orig + 2 and sorted(p % orig for p in q[:orig]) == list(range(orig))
    assert q[orig:] == [0, length - 1]
    visited = sum(int((ref.impulse64(p, 1.0, length, orig_freq, new_freq) != 0).sum()) for p in q[:orig])
    assert visited == int(ref.nonzero_taps(orig_freq, new_freq).sum()) > 0
    # an impulse at either end loses the outputs that would lie before sample 0 / behind the clip's output length
    for p in q[orig:]:
        n = int((ref.impulse64(p, 1.0, length, orig_freq, new_freq) != 0).sum())
        assert 0 < n < visited


@pytest.mark.parametrize("orig_freq,new_freq", ref.PAIRS)
def test_decode_margin_covers_the_filter_support(orig_freq, new_freq):
    assert ref.width(orig_freq, new_freq) <= 256                       # AudioFeatureExtractor._load keeps int(d sr) + 256 samples


def test_edge_lengths_land_on_the_block_edges():
    for orig_freq, new_freq in ref.RANDOM_PAIRS:
        orig, nw = ref.reduced(orig_freq, new_freq)
        lens = ref.edge_lengths(orig_freq, new_freq)
        outs = {ref.out_len(n, orig_freq, new_freq) for n in lens}
        if nw <= orig:                                                 # down-conversion reaches every output length
            assert set(ref.BLOCK_TARGETS) <= outs
        assert {0, 1, 2, 3, orig - 1, orig, orig + 1, 2 * orig + 1, ref.width(orig_freq, new_freq)} <= set(lens)
        assert any(o <= 256 for o in outs) and any(256 < o <= 512 for o in outs) and any(o > 512 for o in outs)


def test_out_len_helper():
    lib = _native.lib()
    for orig_freq, new_freq in ref.PAIRS:
        orig, nw = ref.reduced(orig_freq, new_freq)
        for n in (0, 1, orig - 1, orig, orig + 1, 80000, 2 ** 30):
            want = -((-nw * n) // orig)
            assert lib.sir_resample_out_len(n, orig_freq, new_freq) == (want if want <= INT_MAX else -1), (n, orig_freq, new_freq)
        assert lib.sir_resample_out_len(-1, orig_freq, new_freq) == -1
    assert lib.sir_resample_out_len(10, 0, 16000) == -1 and lib.sir_resample_out_len(10, 16000, 0) == -1
    assert lib.sir_resample_out_len(10, -16000, 16000) == -1 and lib.sir_resample_out_len(10, 16000, -8000) == -1


@pytest.mark.parametrize("length,orig_freq,new_freq", [(INT_MAX, 16000, 48000), (1500000000, 8000, 48000), (2 ** 30, 16000, 44100),
                                                       (INT_MAX // 3 + 1, 16000, 48000)])
def test_out_len_helper_refuses_what_does_not_fit_an_int(length, orig_freq, new_freq):
    assert ref.out_len(length, orig_freq, new_freq) > INT_MAX
    assert _native.lib().sir_resample_out_len(length, orig_freq, new_freq) == -1


@pytest.mark.parametrize("length,orig_freq,new_freq", [(INT_MAX, 48000, 16000), (INT_MAX // 3, 16000, 48000), (INT_MAX, 44100, 44099),
                                                       (INT_MAX, 16000, 16000)])
def test_out_len_helper_is_exact_where_it_fits(length, orig_freq, new_freq):
    want = ref.out_len(length, orig_freq, new_freq)
    assert want <= INT_MAX
    assert _native.lib().sir_resample_out_len(length, orig_freq, new_freq) == want
