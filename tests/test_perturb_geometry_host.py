"""CPU: the WSOLA geometry behind ``sir_wave_perturb`` at every sample rate its entry point accepts, and the float64
contract (tests/wave_perturb_ref.py) at the ends of the tempo range -- no GPU needed.

* the (S, W, O, H) table of tests/perturb_geometry_cases.py against ``ref.geometry``, and for every integer rate from
  8 000 to 24 000 the bounds the kernel's guard (csrc/perturb.hip) relies on: W + S <= 2368 (the LDS window), O <= 288
  (the LDS tail), O % 8 == 0, H >= O, W >= 1;
* the >= 99 % argmin condition of the GPU tests is a property the inputs must have, not a measurement of the kernel: a
  float32 emulation of the search (float32 z and tail, cost summed term by term in float32) picks the float64 argmin on
  >= 99 % of the segments of the GPU tests' rows, with no slack excess;
* ``ref.tempo`` at f = 0.5 and 2: output length, segment count, and the first-minimum rule on an exact tie (an all-zero
  clip, and a burst followed by zeros)."""
import numpy as np
import pytest

import perturb_geometry_cases as cases
import wave_perturb_ref as ref


@pytest.mark.parametrize("sr", sorted(cases.GEOMETRY))
def test_geometry_table(sr):
    S, W, O, H = ref.geometry(sr)
    assert (S, W, O, H) == cases.GEOMETRY[sr] and H == S - O


def test_kernel_guard_invariants_at_every_rate():
    for sr in range(8000, 24001):
        S, W, O, H = ref.geometry(sr)
        assert W + S <= 2368 and O <= 288 and O % 8 == 0 and H >= O and W >= 1 and H == S - O, sr
    assert ref.geometry(24000)[1] + ref.geometry(24000)[0] == 2320 and ref.geometry(24000)[2] == 288


def test_case_lengths_sit_on_the_segment_edges():
    for sr in cases.RATES + [16000]:
        S, W, O, H = ref.geometry(sr)
        lens = cases.lengths_for(sr)
        assert lens == [2 * sr, 0, 1, W // 2, H - 1, H, H + 1, S, 2 * H, 3 * H + 7, 2 * sr - 1] and max(lens) == 2 * sr
        # the longest output a test asks for (tempo 0.5) fits the offsets table and the output buffer
        assert -(-ref.out_len(2 * sr, 0.5) // H) < cases.max_segments(sr)
        assert cases.round_up4(2 * 2 * sr + 4) % 4 == 0 and cases.round_up4(2 * 2 * sr + 4) >= ref.out_len(2 * sr, 0.5) + 4


@pytest.mark.parametrize("sr", [8000, 16000, 24000])
def test_float32_search_stays_inside_the_argmin_cap(sr):
    x = cases.clips(sr)
    segments = hits = 0
    for f in (0.5, 1.15, 2.0):
        for b, n in enumerate(cases.lengths_for(sr)):
            xb = cases.host_f64(x, b, n)
            offs = cases.tempo_offsets_f32(xb, f, sr)
            y, used, costs = ref.tempo(xb, f, sr, offsets=offs)
            assert used == offs and len(costs) == max(len(offs) - 1, 0)
            for c, o in zip(costs, offs[1:]):
                assert c[o] <= c.min() * (1 + 1e-4) + 1e-6, (sr, f, b, o)
                segments += 1
                hits += int(o == int(np.argmin(c)))
    assert segments > 100 and hits >= 0.99 * segments, (hits, segments)


@pytest.mark.parametrize("sr", [8000, 8500, 16000, 24000])
@pytest.mark.parametrize("f", [0.5, 2.0])
def test_tempo_at_the_range_ends(sr, f):
    S, W, O, H = ref.geometry(sr)
    x = cases.host_f64(cases.clips(sr), 0, 2 * sr)
    y, used, costs = ref.tempo(x, f, sr)
    n = int(2 * sr / f + 0.5)
    assert len(y) == n == ref.out_len(2 * sr, f) and len(used) == -(-n // H) and len(costs) == len(used) - 1
    assert used[0] == W // 2 and all(0 <= o < W and len(c) == W for o, c in zip(used[1:], costs))
    assert np.array_equal(y[:H], x[:H])                                  # segment 0 is the clip's first hop as it is
    # exact tie: every candidate of an all-zero clip costs 0, and the first minimum is candidate 0
    zy, zused, zcosts = ref.tempo(np.zeros(2 * sr), f, sr)
    assert len(zy) == n and (zy == 0).all() and zused == [W // 2] + [0] * (len(zused) - 1)
    assert all((c == 0).all() for c in zcosts)


@pytest.mark.parametrize("sr", [8000, 22050, 24000])
def test_tie_clip_has_its_first_minimum_where_it_says(sr):
    W = ref.geometry(sr)[1]
    for a in (1, 40, 65, W - 1):
        x = cases.tie_clip(sr, a).double().numpy()
        y, used, costs = ref.tempo(x, 0.5, sr)
        assert used[1] == a and used[2:] == [0] * (len(used) - 2)
        assert (costs[0][a:] == 0).all() and (costs[0][:a] > 0).all()
        assert cases.tempo_offsets_f32(x, 0.5, sr) == used              # the tie is exact in float32 as well
