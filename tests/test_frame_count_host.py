"""CPU: the conditions the bounds of tests/test_frame_count_gpu.py rest on -- the sweep reaches the frame counts it is meant to,
the signals stay clear of the 1e-10 clamp, and the two float32 yardsticks (the float32 oracle of the forward, the float32 autograd
gradient of the backward) sit where the bounds assume them against float64."""
import numpy as np
import pytest

import frame_count_ref as fc
import frontend_cfg_ref as cref


def test_every_sweep_length_has_its_frame_count():
    for t, n in fc.fwd_cases() + fc.bwd_cases() + [(t, n) for t, n, _ in fc.aug_cases()]:
        assert n > fc.HOP and 1 + n // fc.HOP == t, (t, n)
    for t in fc.FWD_T:
        a, m, z = fc.first_len(t), fc.mid_len(t), fc.last_len(t)
        assert a < m < z and m % 2 == t % 2, (t, a, m, z)
        assert z + 1 == fc.HOP * t and (a == fc.HOP * (t - 1) or t == 2)       # the two ends of the hop
    assert max(fc.FWD_T) <= fc.T_PAD and max(fc.BWD_T) <= fc.T_PAD
    for cfg in fc.GEN_CFGS:
        n_fft, hop, _ = cfg
        cases = fc.gen_cases(cfg)
        assert [t for t, _ in cases] == list(range(fc.gen_min_frames(n_fft, hop), fc.GEN_TMAX + 1))
        assert cref.num_frames(n_fft // 2 + 1, n_fft, hop) == cases[0][0]       # no shorter clip has frames at all
        for t, n in cases:
            assert cref.num_frames(n, n_fft, hop) == t, (cfg, t, n)
        assert fc.GEN_TMAX <= fc.GEN_T_PAD


def test_the_named_edges_occur():
    for name, ts in (("forward", fc.FWD_T), ("backward", fc.BWD_T)):
        for r in (0, 1, 15):
            hits = [t for t in ts if t % 16 == r]
            assert len(hits) >= 3, (name, r, hits)                  # more than a single input per residue
        assert 160 in ts and 161 in ts, name
    assert {2, 3, 16, 17, 18, 32, 33, 48, 49} <= set(fc.BWD_T)      # one, two and three rounds; one and two carries
    assert set(range(2, 177)) == set(fc.FWD_T)
    assert {t for t, _, _ in fc.aug_cases()} == {2, 16, 17, 33, 160, 161}
    by_clip = {}
    for t, n, s in fc.aug_cases():
        by_clip.setdefault((t, n), set()).add(s)
    for (t, n), shifts in by_clip.items():
        assert {n - 1, 1 - n, 511, -513} <= shifts and any(s % 2 == 1 and 0 < s < 511 for s in shifts), (t, n, shifts)
    for cfg in fc.GEN_CFGS:
        ts = {t for t, _ in fc.gen_cases(cfg)}
        assert {16, 17, 63, 64, 65, 128, 129} <= ts, cfg
    # a multiple of the hop (the backward's single-thread fix-up) at every backward frame count but 2, where 512 has no frames
    assert all(fc.first_len(t) == fc.HOP * (t - 1) for t in fc.BWD_T if t > 2)


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_forward_sweep_is_clear_of_the_clamp_and_the_float32_oracle_is_within_its_share(kind):
    ref = fc.fwd_reference(kind)
    print(f"{kind}: smallest mel power {ref['mel_min']:.3e}; float32 oracle against float64, worst over {len(ref['frames'])} clips: "
          f"dB {ref['o32_db'].max():.3e} (T = {ref['frames'][ref['o32_db'].argmax()]}), "
          f"normalised {ref['o32_norm'].max():.3e} (T = {ref['frames'][ref['o32_norm'].argmax()]})")
    assert ref["mel_min"] > 1e3 * 1e-10
    assert ref["o32_db"].max() <= 0.6e-4 and ref["o32_norm"].max() <= 0.6e-4
    assert ref["o32_db"].min() > 0.0                                # (the yardstick is a measurement, not a zero)


@pytest.mark.parametrize("cfg", fc.GEN_CFGS, ids=lambda c: "n%d_h%d_w%d" % c)
def test_general_sweep_is_clear_of_the_clamp_and_the_float32_reference_is_within_its_share(cfg):
    ref = fc.gen_reference(cfg)
    empty = fc.gen_empty_filters(cfg)
    live = [j for j in range(64) if j not in empty]
    lowest = np.inf
    for i, t in enumerate(ref["frames"]):
        lowest = min(lowest, ref["db64"][i, live, :t].min())
        assert (ref["db64"][i, empty, :t] == -100.0).all()          # a filter without a bin is the clamp itself, exactly
    print(f"{cfg}: lowest dB {lowest:.1f}, empty filters {empty}; float32 reference against float64: dB {ref['o32_db'].max():.3e}, "
          f"normalised {ref['o32_norm'].max():.3e}")
    assert lowest > -70.0                                           # 1e3 above the 1e-10 clamp
    assert ref["o32_db"].max() <= 0.6e-4 and ref["o32_norm"].max() <= 0.6e-4


@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_the_float32_gradient_yardstick_is_neither_zero_nor_broken(kind):
    ref = fc.bwd_reference(kind)
    e = ref["e32"]
    cases = fc.bwd_cases()
    print(f"{kind}: clip_error of the float32 autograd gradient over {len(e)} clips: min {e.min():.2e} (L = {cases[e.argmin()][1]}), "
          f"median {np.median(e):.2e}, max {e.max():.2e} (L = {cases[e.argmax()][1]})")
    assert e.min() >= 1e-6 and e.max() <= 1e-4
    for g, (_, n) in zip(ref["g64"], cases):
        assert g.shape == (n,) and g.abs().max() > 0


def test_augmented_sweep_is_clear_of_the_clamp():
    ref = fc.aug_reference()
    e = ref["e32"][~ref["constant"] & ~ref["dead"]]
    print(f"augmented clips: lowest dB {ref['db_min']:.1f}, constant tiles {int(ref['constant'].sum())}, clips shifted out "
          f"altogether {int(ref['dead'].sum())}; float32 autograd "
          f"clip_error min {e.min():.2e} median {np.median(e):.2e} max {e.max():.2e}")
    assert ref["db_min"] > -70.0
    assert np.isfinite(e).all() and e.min() > 0.0
    assert int(ref["dead"].sum()) == 1                             # (T = 2, L = 513, shift -513)


def test_the_fold_of_the_last_padded_sample_is_measurable():
    """With ``dout`` on the last frame alone the part of the gradient that comes back from the last padded sample stands clear of
    float32 rounding (1e-7 of the rms): the condition test_backward_folds_the_last_padded_sample rests on."""
    ref, cases = fc.fold_reference("f32"), fc.fold_cases()
    assert len([t for t, _ in cases if (t - 1) % 16 == 0]) >= 3     # frame T - 1 opens a round: the block was written a round earlier
    rel = np.array([abs(ref["fold"][i]) / ref["g64"][i].pow(2).mean().sqrt().item() for i in range(len(cases))])
    print(f"|fold| / rms over {len(cases)} clips: min {rel.min():.2e}, median {np.median(rel):.2e}, max {rel.max():.2e}")
    assert np.median(rel) >= 1e-6 and rel.max() >= 1e-5
