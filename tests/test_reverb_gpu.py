"""GPU: sir_wave_reverb_mix (HipFeaturizer.reverb_mix) against the float64 oracle of tests/reverb_ref.py.

Shapes cross every boundary of a 512-sample partition and a 1024-point block.  The reverb bound is the issue's condition, max
|out - oracle| <= 1e-5 |x|_inf |h|_1 per row (about 170 float32 unit roundoffs of the largest value the output can take); every
case prints the largest ratio it saw (pytest -s) ahead of its assertion."""
import functools

import numpy as np
import pytest
import torch

import reverb_ref as ref
from reverb_call import NAN, bank as _bank, call, i32 as _i32
from sir_amd import _native, ops, synth
from sir_amd.sound_bank import SoundBank

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 511, 512, 513, 1023, 1025, 1537, 5000, 5000, 4097]
MAX_LEN, STRIDE = 5000, 5008
RIR_K = [1, 2, 511, 512, 513, 1025, 3000, 8192]
RIR_INDEX = [3, 0, 1, 2, 3, 4, 5, 6, 7, -1, 7]                   # -1 and repeated RIRs (3 and 7)


@pytest.fixture(scope="module")
def fz():
    from sir_amd.featurizer import get_featurizer
    return get_featurizer()


@pytest.fixture(scope="module")
def data():
    """clips (float32 and PCM16), RIRs and noises shared by the cases; never modified"""
    gen = np.random.default_rng(2024)
    x = synth.synth_clips(len(LENGTHS), MAX_LEN, seed=31)
    rirs = []
    for k in RIR_K:
        h = (gen.standard_normal(k) * np.exp(-4.0 * np.arange(k) / max(k, 64))).astype(np.float32)
        h[0] = 1.0
        rirs.append(h)
    noises = [(0.2 * gen.standard_normal(700)).astype(np.float32), synth.coloured_noise(6001, gen).numpy(),
              np.zeros(40, dtype=np.float32), (0.01 * gen.standard_normal(3)).astype(np.float32)]
    return {"x": x, "x16": synth.to_int16(x), "rirs": rirs, "noises": noises}


_call = functools.partial(call, max_len=MAX_LEN, out_stride=STRIDE)     # the file's geometry; a call may still name its own


def _wave(x, fill=None):
    """[B][STRIDE] on the GPU; `fill` behind each row's length (NaN for float32, a loud value for PCM16)"""
    w = torch.zeros((len(LENGTHS), STRIDE), dtype=x.dtype)
    w[:, :MAX_LEN] = x
    if fill is not None:
        for b, n in enumerate(LENGTHS):
            w[b, n:] = fill
    return w.cuda()


def _f64(x):
    return x.double().numpy() / (32768.0 if x.dtype == torch.int16 else 1.0)


def _check_tail(out, sentinel_nan=True):
    o = out.cpu()
    for b, n in enumerate(LENGTHS):
        assert torch.isfinite(o[b, :MAX_LEN]).all(), b
        assert (o[b, n:MAX_LEN] == 0).all(), b
        assert torch.isnan(o[b, MAX_LEN:]).all(), b              # columns >= max_len untouched


def _reverb_ratio(out, want, x64, rirs, index):
    worst = 0.0
    for b, n in enumerate(LENGTHS):
        if n == 0 or index[b] < 0:
            continue
        bound = np.abs(x64[b, :n]).max() * np.abs(rirs[index[b]].astype(np.float64)).sum()
        err = np.abs(out[b, :n].double().numpy() - want[b][0]).max()
        worst = max(worst, err / bound)
    return worst


def test_reverb_only(fz, data):
    w = _wave(data["x"], NAN)
    rc, out, gain = _call(fz, w, LENGTHS, rir=_bank(data["rirs"], NAN), rir_index=RIR_INDEX)
    assert rc == 0
    ops.check_status()
    want = ref.mix_batch(_f64(data["x"]), LENGTHS, data["rirs"], RIR_INDEX)
    _check_tail(out)
    ratio = _reverb_ratio(out.cpu(), want, _f64(data["x"]), data["rirs"], RIR_INDEX)
    print(f"reverb only: max |out - oracle| / (|x|_inf |h|_1) = {ratio:.3e}")
    assert ratio <= 1e-5
    assert torch.equal(out[9, :5000], w[9, :5000])                # rir -1: a copy
    assert not gain.any()


def test_every_rir_on_the_longest_clips(fz, data):
    """each K against L = 5000 and L = 4097 (ten blocks; the last one partial), each RIR used by two rows"""
    idx = [-1, -1, -1, 0, 1, 2, 3, 4, 5, 6, 7]
    lens = [0, 1, 511, 5000, 4097, 5000, 4097, 5000, 4097, 5000, 4097]
    x = data["x"]
    w = torch.full((len(lens), STRIDE), NAN)
    for b, n in enumerate(lens):
        w[b, :n] = x[b, :n]
    rc, out, _ = _call(fz, w.cuda(), lens, rir=_bank(data["rirs"], NAN), rir_index=idx)
    assert rc == 0
    ops.check_status()
    want = ref.mix_batch(_f64(x), lens, data["rirs"], idx)
    worst = 0.0
    for b, n in enumerate(lens):
        if idx[b] >= 0:
            bound = np.abs(_f64(x)[b, :n]).max() * np.abs(data["rirs"][idx[b]].astype(np.float64)).sum()
            worst = max(worst, np.abs(out[b, :n].cpu().double().numpy() - want[b][0]).max() / bound)
    print(f"every K at L = 5000 / 4097: max ratio = {worst:.3e}")
    assert worst <= 1e-5


def test_bit_exact_rows(fz, data):
    none = [-1] * len(LENGTHS)
    for x in (data["x"], data["x16"]):
        w = _wave(x, NAN if x.dtype == torch.float32 else 30000)
        rc, out, gain = _call(fz, w, LENGTHS, rir=_bank(data["rirs"]), rir_index=none, noise=_bank(data["noises"]),
                              noise_index=none, noise_offset=[5] * len(LENGTHS), snr_db=[NAN] * len(LENGTHS))   # snr unread at -1
        assert rc == 0
        ops.check_status()
        deq = x.float() / 32768.0 if x.dtype == torch.int16 else x
        for b, n in enumerate(LENGTHS):
            assert torch.equal(out[b, :n].cpu(), deq[b, :n]), b
        _check_tail(out)
        rc, out2, _ = _call(fz, w, LENGTHS)                       # both index vectors NULL
        assert rc == 0 and torch.equal(out2[:, :MAX_LEN], out[:, :MAX_LEN])


def test_noise(fz, data):
    nidx = [0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 1]                      # M = 700 (seven wraps at L = 5000) and M = 6001 > L
    offs = [0, 699, 697, 6000, 1, 350, 17, 697, 697, 0, 5999]
    snrs = [0.0, 20.0, -5.0, 0.0, 20.0, -5.0, 0.0, 20.0, -5.0, 0.0, 20.0]
    w = _wave(data["x"], NAN)
    rc, out, gain = _call(fz, w, LENGTHS, noise=_bank(data["noises"], NAN), noise_index=nidx, noise_offset=offs, snr_db=snrs)
    assert rc == 0
    ops.check_status()
    want = ref.mix_batch(_f64(data["x"]), LENGTHS, None, None, data["noises"], nidx, offs, snrs)
    _check_tail(out)
    worst_g = worst_o = 0.0
    for b, n in enumerate(LENGTHS):
        o, y, g, used = want[b]
        if n == 0:
            assert gain[b] == 0.0
            continue
        worst_g = max(worst_g, abs(gain[b] - g) / g)
        bound = np.abs(y).max() + g * np.abs(used).max()
        worst_o = max(worst_o, np.abs(out[b, :n].cpu().double().numpy() - o).max() / bound)
    print(f"noise: max relative gain error = {worst_g:.3e}, max |out - oracle| / (|y|_inf + g |v|_inf) = {worst_o:.3e}")
    assert worst_g <= 1e-5 and worst_o <= 1e-5


def test_silent_clip_and_silent_noise(fz, data):
    x = data["x"].clone()
    x[8] = 0.0                                                     # a silent clip with a live noise
    nidx = [0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 3]                      # row 9: the all-zero noise; row 10: M = 3
    rc, out, gain = _call(fz, _wave(x, NAN), LENGTHS, noise=_bank(data["noises"], NAN), noise_index=nidx,
                          noise_offset=[3] * len(LENGTHS), snr_db=[10.0] * len(LENGTHS))
    assert rc == 0
    ops.check_status()
    _check_tail(out)
    assert gain[8] == 0.0 and gain[9] == 0.0 and gain[0] == 0.0 and gain[10] > 0.0
    assert not out[8, :MAX_LEN].any()
    assert torch.equal(out[9, :5000].cpu(), x[9, :5000])
    want = ref.mix_row(x[10, :4097].double().numpy(), None, data["noises"][3], 3, 10.0)
    assert abs(gain[10] - want[2]) <= 1e-5 * want[2]


def test_both_effects_on_int16(fz, data):
    nidx = [1, 0, -1, 0, 1, 0, 0, 1, 0, 0, 0]
    offs = [0, 5, 0, 697, 6000, 1, 2, 3, 697, 4, 5]
    snrs = [0.0, 20.0, 0.0, -5.0, 0.0, 20.0, -5.0, 0.0, 20.0, -5.0, 0.0]
    w = _wave(data["x16"], 30000)
    rc, out, gain = _call(fz, w, LENGTHS, rir=_bank(data["rirs"], NAN), rir_index=RIR_INDEX, noise=_bank(data["noises"], NAN),
                          noise_index=nidx, noise_offset=offs, snr_db=snrs)
    assert rc == 0
    ops.check_status()
    x64 = _f64(data["x16"])
    want = ref.mix_batch(x64, LENGTHS, data["rirs"], RIR_INDEX, data["noises"], nidx, offs, snrs)
    _check_tail(out)
    worst = worst_g = 0.0
    for b, n in enumerate(LENGTHS):
        if n == 0:
            continue
        o, y, g, used = want[b]
        h1 = np.abs(data["rirs"][RIR_INDEX[b]].astype(np.float64)).sum() if RIR_INDEX[b] >= 0 else 1.0
        bound = np.abs(x64[b, :n]).max() * h1 + (g * np.abs(used).max() if used is not None else 0.0)
        worst = max(worst, np.abs(out[b, :n].cpu().double().numpy() - o).max() / bound)
        if used is not None:
            worst_g = max(worst_g, abs(gain[b] - g) / g)
    print(f"reverb + noise on PCM16: max error / bound = {worst:.3e}, max relative gain error = {worst_g:.3e}")
    assert worst <= 1e-5 and worst_g <= 1e-5


def test_deterministic_and_row_independent(fz, data):
    nidx = [1, 0, -1, 0, 1, 0, 0, 1, 0, 0, 0]
    args = dict(noise_offset=[7, 5, 0, 697, 6000, 1, 2, 3, 697, 4, 5], snr_db=[3.0] * len(LENGTHS))
    rirs, noises = _bank(data["rirs"]), _bank(data["noises"])
    w = _wave(data["x"])
    _, a, ga = _call(fz, w, LENGTHS, rir=rirs, rir_index=RIR_INDEX, noise=noises, noise_index=nidx, **args)
    _, b, gb = _call(fz, w, LENGTHS, rir=rirs, rir_index=RIR_INDEX, noise=noises, noise_index=nidx, **args)
    assert torch.equal(a[:, :MAX_LEN], b[:, :MAX_LEN]) and np.array_equal(ga, gb)
    perm = [10, 3, 8, 0, 9, 1, 7, 2, 6, 4, 5]
    pick = lambda v: [v[i] for i in perm]
    _, c, gc = _call(fz, w[perm].contiguous(), pick(LENGTHS), rir=rirs, rir_index=pick(RIR_INDEX), noise=noises,
                     noise_index=pick(nidx), noise_offset=pick(args["noise_offset"]), snr_db=pick(args["snr_db"]))
    assert torch.equal(c[:, :MAX_LEN], a[perm][:, :MAX_LEN]) and np.array_equal(gc, ga[perm])
    ops.check_status()


def test_bad_rows_zero_only_themselves(fz, data):
    rirs, noises = _bank(data["rirs"]), _bank(data["noises"])
    nidx = [0] * len(LENGTHS)
    offs, snrs = [1] * len(LENGTHS), [6.0] * len(LENGTHS)
    w = _wave(data["x"])
    _, good, _ = _call(fz, w, LENGTHS, rir=rirs, rir_index=RIR_INDEX, noise=noises, noise_index=nidx, noise_offset=offs, snr_db=snrs)
    ops.check_status()
    k0 = rirs[1].clone()
    k0[6] = 0                                                      # RIR 6 (row 7 uses it) claims K = 0
    cases = [(8, dict(rir_index=RIR_INDEX[:8] + [len(RIR_K)] + RIR_INDEX[9:])),
             (7, dict(rir_lengths=k0, max_rir_len=8192)),
             (5, dict(snr_db=snrs[:5] + [NAN] + snrs[6:])),
             (4, dict(noise_index=nidx[:4] + [-2] + nidx[5:]))]
    for row, change in cases:
        kw = dict(rir=rirs, rir_index=RIR_INDEX, noise=noises, noise_index=nidx, noise_offset=offs, snr_db=snrs)
        kw.update(change)
        rc, out, _ = _call(fz, w, LENGTHS, **kw)
        assert rc == 0
        assert not out[row, :MAX_LEN].any(), row
        others = [b for b in range(len(LENGTHS)) if b != row]
        assert torch.equal(out[others][:, :MAX_LEN], good[others][:, :MAX_LEN]), row
        with pytest.raises(_native.SirError, match="sir_wave_reverb_mix"):
            ops.check_status()
        ops.check_status()                                        # raised once: the word is cleared


def test_bad_call_arguments_launch_nothing(fz, data):
    rirs = _bank(data["rirs"], extra=16)
    w = _wave(data["x"])
    sentinel = torch.full((len(LENGTHS), STRIDE), 7.0, device="cuda")
    rc, out, _ = _call(fz, w, LENGTHS, rir=rirs, rir_index=RIR_INDEX, max_rir_len=8193, out=sentinel)
    assert rc == _native.SIR_EINVAL and (out == 7.0).all()
    rc, out, _ = _call(fz, w, LENGTHS, rir=rirs, rir_index=RIR_INDEX, ws_bytes=8, out=sentinel)
    assert rc != 0 and rc != _native.SIR_EINVAL and (out == 7.0).all()          # SIR_ENOMEM
    rc, out, _ = _call(fz, w, LENGTHS, rir=rirs, rir_index=RIR_INDEX, out=w)    # out must not overlap wave
    assert rc == _native.SIR_EINVAL
    assert _native.lib().sir_reverb_workspace_bytes(fz.handle, 4, 100, 8193) == 0
    ops.check_status()


def test_prefetcher_end_to_end(fz, data):
    from sir_amd.pipeline import FeaturePrefetcher
    gen = np.random.default_rng(5)
    lens = [4000, 9000, 5121, 7777, 8192, 6000]
    x = synth.synth_clips(6, 9000, seed=9)
    for b, n in enumerate(lens):
        x[b, n:] = 0
    rir = SoundBank([synth.synthetic_rir(t, rng=gen) for t in (0.05, 0.2, 0.4)], kind="rir")
    noise = SoundBank([synth.coloured_noise(3000, gen), synth.coloured_noise(20000, gen, exponent=2.0)])
    ri, ni = [0, 1, 2, -1, 2, 1], [0, 1, -1, 0, 1, 0]
    off, snr = [2999, 5, 0, 100, 19000, 1], [10.0, 0.0, 0.0, 20.0, 5.0, -5.0]
    shift = [0, 300, -200, 0, 50, 0]
    wave, lengths = x.cuda(), _i32(lens)
    kw = dict(rir=rir, noise=noise, rir_index=torch.tensor(ri, dtype=torch.int32), noise_index=torch.tensor(ni, dtype=torch.int32),
              noise_offset=torch.tensor(off, dtype=torch.int32), snr_db=torch.tensor(snr))
    for sh in (None, shift):
        pre = FeaturePrefetcher(t_pad=24, **kw, **({"shift": torch.tensor(sh, dtype=torch.int32)} if sh else {}))
        pre.submit(wave, lengths)
        got = pre.get().clone()
        pre.release()
        torch.cuda.synchronize()
        ops.check_status()
        xs = x.double().numpy()
        if sh:                                                    # the shift stays ahead of the reverb
            for b, n in enumerate(lens):
                row = np.zeros(9000)
                s = sh[b]
                row[max(s, 0):n + min(s, 0)] = xs[b, max(-s, 0):n - max(s, 0)]
                xs[b] = row
        want = ref.mix_batch(xs, lens, [r[:k].numpy() for r, k in zip(rir.data, rir.host_lengths)], ri,
                             [v[:k].numpy() for v, k in zip(noise.data, noise.host_lengths)], ni, off, snr)
        oracle = torch.zeros(6, 9000)
        for b, n in enumerate(lens):
            oracle[b, :n] = torch.from_numpy(want[b][0]).float()
        feats = fz(oracle.cuda(), lengths, t_pad=24)
        err = ((got - feats).abs() / feats.abs().clamp(min=1.0)).max().item()
        print(f"prefetcher (shift {'on' if sh else 'off'}): max feature error = {err:.3e}")
        assert err <= 1e-4
    plain = fz(wave, lengths, t_pad=24)
    pre = FeaturePrefetcher(t_pad=24)
    pre.submit(wave, lengths)
    same = pre.get().clone()
    pre.release()
    torch.cuda.synchronize()
    assert torch.equal(same, plain)


def test_batch_pipeline_features(fz, data):
    """BatchPipeline.features runs the same stage on its slot stream"""
    from sir_amd.models.models import CNNAudioGRU
    from sir_amd.pipeline import BatchPipeline
    gen = np.random.default_rng(6)
    rir = SoundBank([synth.synthetic_rir(0.1, rng=gen)], kind="rir")
    x = synth.synth_clips(4, 6000, seed=10).cuda()
    idx = torch.tensor([0, -1, 0, 0], dtype=torch.int32)
    want = fz(fz.reverb_mix(x, rir=rir, rir_index=idx), t_pad=24)
    torch.cuda.synchronize()
    model = CNNAudioGRU(num_classes=31).cuda().eval()
    pipe = BatchPipeline(model, n_streams=2)
    got = pipe.features(0, x, t_pad=24, rir=rir, rir_index=idx)
    pipe.synchronize()
    assert torch.equal(got, want)
    ops.check_status()
