"""GPU: the waveform front end (csrc/frontend.hip) against the float64 references of tests/frontend_edge_ref.py -- the
resampler at every tap of every phase of sixteen rate pairs and at the clip and block edges, the channel mix-down bit for
bit, and the two batch-assembly kernels (``sir_gather_features``, ``sir_mix_features``) beyond one pass of their grid-stride
loops.  Every bound is derived in frontend_edge_ref.py's docstring (mix: tests/test_recipe_gpu.py); none comes from the
device.  tests/test_frontend_edge_host.py holds the conditions these comparisons rest on.

Measured on MI355X (worst err / bound; each test prints its own): impulses 0.497 with 0 taps that are not the nearest float32,
random clips 0.327 (12000 -> 16000, int16), mono float32 0.770 (3 channels), mono int16 and gather 0 differing bits, mix 0.892."""
import numpy as np
import pytest
import torch

import frontend_edge_ref as ref
import recipe_ref
from sir_amd import _native, ops, train_ops
from sir_amd.feature_store import FeatureStore
from sir_amd.featurizer import HipFeaturizer, get_featurizer

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = ref.U
SENTINEL = 0x7FC12345                      # a NaN with a payload: a float the kernels never produce


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- a. impulse response: every tap of every phase ---------------------------------------------------------------------------
@pytest.mark.parametrize("orig_freq,new_freq", ref.PAIRS)
def test_impulse_response_every_tap(orig_freq, new_freq):
    fz = get_featurizer()
    length, q = ref.impulse_case(orig_freq, new_freq)
    rows, t_out = len(q), ref.out_len(length, orig_freq, new_freq)
    h = ref.h64(orig_freq, new_freq, np.arange(t_out)[None, :], np.asarray(q)[:, None])       # [rows, t_out], amplitude 1
    lengths = torch.full((rows,), length, dtype=torch.int32, device=DEV)
    for dtype, amp, poison in ((np.float32, 1.0, np.nan), (np.int16, 16384, 32767)):
        x = np.zeros((rows, length + 3), dtype=dtype)
        x[:, length:] = poison                                          # behind the clips' length: never read
        x[np.arange(rows), q] = amp
        y, out_len = fz.resample(_dev(x), orig_freq, new_freq, lengths)
        y, out_len = y.cpu().numpy(), out_len.cpu().numpy()
        assert (out_len == t_out).all()
        assert y.shape[1] >= t_out and (y[:, t_out:] == 0).all()
        want = h * (1.0 if dtype == np.float32 else 0.5)
        got = y[:, :t_out].astype(np.float64)
        err, bound = np.abs(got - want), ref.impulse_bound(want)
        not_nearest = int((y[:, :t_out] != want.astype(np.float32)).sum())
        print(f"impulse {orig_freq}->{new_freq} {np.dtype(dtype).name}: {int((want != 0).sum())} taps met, {not_nearest} not the "
              f"nearest float32, worst err / bound {(err / bound).max():.3f}")
        assert (err <= bound).all()
        assert (got[want == 0] == 0).all()


# ---- b. random signals at the length edges ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_refs():
    """pair -> dtype name -> per row (y, bound), computed once."""
    out = {}
    for pair in ref.RANDOM_PAIRS:
        case = ref.random_case(*pair)
        per = {}
        for name, scale in (("f32", 1.0), ("i16", 1.0 / 32768.0)):
            rows = []
            for b, n in enumerate(case["used"]):
                y, s = ref.resample64(case[name][b, :n].astype(np.float64) * scale, *pair)
                rows.append((y, ref.resample_bound(s, *pair)))
            per[name] = rows
        out[pair] = (case, per)
    return out


@pytest.mark.parametrize("name", ["f32", "i16"])
@pytest.mark.parametrize("orig_freq,new_freq", ref.RANDOM_PAIRS)
def test_random_clips_at_the_length_edges(random_refs, orig_freq, new_freq, name):
    fz = get_featurizer()
    case, per = random_refs[(orig_freq, new_freq)]
    x, lengths = _dev(case[name]), _dev(case["lengths"])
    y, out_len = fz.resample(x, orig_freq, new_freq, lengths)
    yc, out_len = y.cpu().numpy(), out_len.cpu().numpy()
    worst = 0.0
    for b, n in enumerate(case["used"]):
        want, bound = per[name][b]
        t = ref.out_len(n, orig_freq, new_freq)
        assert int(out_len[b]) == t == len(want), (b, n)
        assert (yc[b, t:] == 0).all(), (b, n)                           # zero behind the clip's output; all of it for an empty clip
        if t:
            err = np.abs(yc[b, :t].astype(np.float64) - want)
            ratio = float((err / np.maximum(bound, 1e-300)).max())
            assert (err <= bound).all(), (b, n, ratio)
            worst = max(worst, ratio)
        # the row alone, in a buffer cut to its own length: another grid, the same bits
        alone, alone_len = fz.resample(x[b:b + 1, :max(n, 1)].contiguous(), orig_freq, new_freq, lengths[b:b + 1])
        assert int(alone_len[0]) == t
        assert torch.equal(_bits(alone[0, :t]), _bits(y[b, :t])), (b, n)
    assert case["lengths"][-1] == -1000 and int(out_len[-1]) == 0 and (yc[-1] == 0).all()
    assert case["lengths"][-2] == x.shape[1] + 1000 and int(out_len[-2]) == ref.out_len(x.shape[1], orig_freq, new_freq)
    print(f"random {orig_freq}->{new_freq} {name}: worst err / bound {worst:.3f}")


def test_mono_negative_frame_count_is_an_empty_clip():
    fz = get_featurizer()
    pcm = torch.full((2, 600), 32767, dtype=torch.int16, device=DEV)
    out = fz.mix_to_mono(pcm, 2, torch.tensor([-1000, 300], dtype=torch.int32, device=DEV)).cpu()
    assert (out[0] == 0).all() and (out[1] == 32767.0 / 32768.0).all()


# ---- c. strides, truncation, sentinels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "i16"])
@pytest.mark.parametrize("orig_freq,new_freq", [(44100, 8000), (11025, 16000)])
def test_resample_abi_strides_truncation_and_untouched_columns(random_refs, orig_freq, new_freq, name):
    fz, lib = get_featurizer(), _native.lib()
    case, per = random_refs[(orig_freq, new_freq)]
    bsz, max_len = case[name].shape
    poison = np.nan if name == "f32" else 32767
    wide = np.full((bsz, max_len + 9), poison, dtype=case[name].dtype)
    wide[:, 4:4 + max_len] = case[name]
    wide = _dev(wide)
    wave = wide[:, 4:4 + max_len]                                       # wave_stride = max_len + 9 > max_len
    assert wave.stride(0) == max_len + 9
    lengths = _dev(case["lengths"])
    dt = _native.WAVE_F32 if name == "f32" else _native.WAVE_I16
    max_out = 300
    targets = [ref.out_len(n, orig_freq, new_freq) for n in case["used"]]
    assert any(0 < t < max_out for t in targets) and any(t > max_out for t in targets)
    outs = []
    for with_lengths in (True, False):
        out = _sentinel(bsz, max_out + 5)
        out_len = torch.full((bsz,), -7, dtype=torch.int32, device=DEV)
        rc = lib.sir_resample(fz.handle, wave.data_ptr(), dt, wave.stride(0), lengths.data_ptr(), bsz, max_len, orig_freq, new_freq,
                              out.data_ptr(), max_out + 5, max_out, out_len.data_ptr() if with_lengths else None,
                              _native.current_stream_ptr())
        _native.check(rc, "sir_resample")
        outs.append((out, out_len.cpu().numpy()))
    (out, out_len), (out_null, untouched) = outs
    assert (untouched == -7).all()
    assert torch.equal(_bits(out), _bits(out_null))                     # out_lengths == NULL: the same samples
    assert (_bits(out[:, max_out:]) == SENTINEL).all()                  # nothing written at or beyond max_out_len
    oc = out.cpu().numpy()
    for b, n in enumerate(case["used"]):
        want, bound = per[name][b]
        t = min(targets[b], max_out)
        assert int(out_len[b]) == t, (b, n)
        assert (np.abs(oc[b, :t].astype(np.float64) - want[:t]) <= bound[:t]).all(), (b, n)
        assert (oc[b, t:max_out] == 0).all(), (b, n)


@pytest.mark.parametrize("channels", [1, 3, 64])
def test_mono_abi_strides_and_untouched_columns(channels):
    fz, lib = get_featurizer(), _native.lib()
    rng = np.random.Generator(np.random.PCG64(channels))
    max_frames = 261
    frames = [261, 256, 1, 0, 900, -5]
    pcm = np.full((len(frames), max_frames * channels + 6), 32767, dtype=np.int16)
    want = np.zeros((len(frames), max_frames), dtype=np.float32)
    for b, n in enumerate(frames):
        n = min(max(n, 0), max_frames)
        clip = rng.integers(-32768, 32768, (n, channels)).astype(np.int16)
        pcm[b, :n * channels] = clip.reshape(-1)
        want[b, :n] = ref.mono_i16_exact(clip)
    pcm = _dev(pcm)
    out = _sentinel(len(frames), max_frames + 5)
    rc = lib.sir_mix_to_mono(fz.handle, pcm.data_ptr(), _native.WAVE_I16, channels, pcm.stride(0), _dev(np.asarray(frames, dtype=np.int32)).data_ptr(),
                             len(frames), max_frames, out.data_ptr(), max_frames + 5, _native.current_stream_ptr())
    _native.check(rc, "sir_mix_to_mono")
    assert (_bits(out[:, max_frames:]) == SENTINEL).all()
    assert np.array_equal(out[:, :max_frames].cpu().numpy().view(np.int32), want.view(np.int32))


def test_refused_calls_write_nothing():
    fz, lib = get_featurizer(), _native.lib()
    h, st = fz.handle, _native.current_stream_ptr()
    wave = torch.zeros((2, 64), dtype=torch.float32, device=DEV)
    lengths = torch.full((2,), 64, dtype=torch.int32, device=DEV)
    out = _sentinel(2, 64)
    out_len = torch.full((2,), -7, dtype=torch.int32, device=DEV)

    def resample(dtype=_native.WAVE_F32, batch=2, max_len=64, orig_freq=22050, new_freq=16000, max_out=47):
        return lib.sir_resample(h, wave.data_ptr(), dtype, 64, lengths.data_ptr(), batch, max_len, orig_freq, new_freq, out.data_ptr(), 64,
                                max_out, out_len.data_ptr(), st)

    def mono(dtype=_native.WAVE_F32, channels=2, batch=2, max_frames=32):
        return lib.sir_mix_to_mono(h, wave.data_ptr(), dtype, channels, 64, lengths.data_ptr(), batch, max_frames, out.data_ptr(), 64, st)

    refused = [resample(dtype=7), resample(dtype=-1), resample(orig_freq=16000), resample(orig_freq=0), resample(new_freq=0),
               resample(orig_freq=-22050), resample(batch=0), resample(batch=-1), resample(max_len=0), resample(max_out=0),
               resample(max_out=-3), mono(channels=0), mono(channels=65), mono(channels=-1), mono(dtype=7), mono(batch=0),
               mono(max_frames=0), mono(max_frames=-1)]
    assert refused == [_native.SIR_EINVAL] * len(refused)
    torch.cuda.synchronize()
    assert (_bits(out) == SENTINEL).all() and (out_len == -7).all()
    assert mono(channels=64, max_frames=1) == _native.SIR_OK and resample() == _native.SIR_OK       # the same calls, accepted
    torch.cuda.synchronize()
    assert (out[:, 0] == 0).all() and (out_len.cpu() == 47).all()


# ---- d. the handle's table cache -----------------------------------------------------------------------------------------------
def test_table_cache_returns_each_pairs_own_table():
    fz = HipFeaturizer()                                                # its own handle: no table built yet
    g = torch.Generator().manual_seed(4)
    x = (0.3 * torch.randn(3, 1500, generator=g)).to(DEV)
    lengths = torch.tensor([1500, 1499, 441], dtype=torch.int32, device=DEV)
    a, b, c, d = (44100, 16000), (22050, 8000), (48000, 16000), (24000, 8000)
    first = {}
    for pair in (a, b, a, c, b, d, c, a):
        y, n = fz.resample(x, pair[0], pair[1], lengths)
        if pair not in first:
            first[pair] = (y, n)
        else:
            assert torch.equal(_bits(y), _bits(first[pair][0])) and torch.equal(n, first[pair][1]), pair
    for p, q in ((a, b), (c, d)):                                       # the same reduced ratio: the same filter
        assert ref.reduced(*p) == ref.reduced(*q)
        assert torch.equal(_bits(first[p][0]), _bits(first[q][0])) and torch.equal(first[p][1], first[q][1])
    assert not torch.equal(first[a][0][:, :400], first[c][0][:, :400])
    torch.cuda.synchronize()                                            # before the handle and its tables go


# ---- e. what the file route relies on ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig_freq,new_freq", [(96000, 8000), (44100, 16000)])
def test_truncating_the_decode_keeps_the_kept_output(orig_freq, new_freq):
    """``AudioFeatureExtractor._load`` keeps int(d sr) + 256 samples; the first int(d new) outputs do not depend on the rest."""
    fz = get_featurizer()
    d = 0.05
    keep = int(d * orig_freq) + 256
    g = torch.Generator().manual_seed(orig_freq)
    x = (0.3 * torch.randn(1, 3 * keep, generator=g)).to(DEV)
    whole, _ = fz.resample(x, orig_freq, new_freq)
    cut, _ = fz.resample(x[:, :keep].contiguous(), orig_freq, new_freq)
    kept = int(d * new_freq)
    assert cut.shape[1] >= kept > 0
    assert torch.equal(_bits(cut[:, :kept]), _bits(whole[:, :kept]))
    assert not torch.equal(cut[:, :cut.shape[1]], whole[:, :cut.shape[1]])          # (the cut is felt behind it)


# ---- f. mono -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", ref.MONO_CHANNELS)
def test_mono_int16_is_the_exact_quotient(channels):
    fz = get_featurizer()
    rng = np.random.Generator(np.random.PCG64(100 + channels))
    max_frames = 300
    frames = [300, 300, 257, 350, 300, 0]                               # full scale both ways, short, clamped, random, empty
    pcm = np.full((len(frames), max_frames * channels), 32767, dtype=np.int16)
    want = np.zeros((len(frames), max_frames), dtype=np.float32)
    for b, n in enumerate(frames):
        n = min(n, max_frames)
        clip = rng.integers(-32768, 32768, (n, channels)).astype(np.int16)
        if b < 2:
            clip[:] = (-32768, 32767)[b]
        pcm[b, :n * channels] = clip.reshape(-1)
        want[b, :n] = ref.mono_i16_exact(clip)
    out = fz.mix_to_mono(_dev(pcm), channels, _dev(np.asarray(frames, dtype=np.int32))).cpu().numpy()
    differ = out.view(np.int32) != want.view(np.int32)
    assert not differ.any(), (int(differ.sum()), out[differ][:8], want[differ][:8])
    assert (out[0] == -1.0).all() and (out[2, 257:] == 0).all()


@pytest.mark.parametrize("channels", ref.MONO_CHANNELS)
def test_mono_float32_within_one_rounding_of_the_magnitude_sum(channels):
    fz = get_featurizer()
    rng = np.random.Generator(np.random.PCG64(200 + channels))
    max_frames = 300
    frames = [300, 257, 1, 350]
    pcm = np.full((len(frames), max_frames * channels), np.nan, dtype=np.float32)
    out = fz.mix_to_mono(_dev(pcm), channels, torch.zeros(len(frames), dtype=torch.int32, device=DEV)).cpu()
    assert (out == 0).all()                                             # nothing read behind a count of 0
    clips = []
    for b, n in enumerate(frames):
        n = min(n, max_frames)
        clip = rng.standard_normal((n, channels)).astype(np.float32)
        clip[:, channels // 2] *= 1e4                                   # one channel 1e4 times the others
        pcm[b, :n * channels] = clip.reshape(-1)
        clips.append(clip)
    out = fz.mix_to_mono(_dev(pcm), channels, _dev(np.asarray(frames, dtype=np.int32))).cpu().numpy()
    worst = 0.0
    for b, clip in enumerate(clips):
        n = len(clip)
        want, bound = ref.mono_f32(clip)
        err = np.abs(out[b, :n].astype(np.float64) - want)
        assert (err <= bound).all(), (b, float((err / bound).max()))
        assert (out[b, n:] == 0).all()
        worst = max(worst, float((err / bound).max()))
    print(f"mono float32, {channels} channels: worst err / bound {worst:.3f}")


# ---- g. gather beyond one pass of the grid ---------------------------------------------------------------------------------
def _zero_band(t, dim, start, size, extent):
    if size > 0:
        lo, hi = max(start, 0), min(max(start + size, 0), extent)
        if hi > lo:
            t.narrow(dim, lo, hi - lo).zero_()


@pytest.mark.parametrize("n_mels,t_pad", [(64, 260), (64, 2056), (128, 200), (64, 200), (3, 12), (1, 4)])
def test_gather_every_band_start_and_width(n_mels, t_pad):
    ops.check_status()
    g = torch.Generator().manual_seed(n_mels * 10000 + t_pad)
    host = torch.randn(7, n_mels, t_pad, generator=g)
    store = FeatureStore.from_tensors(host.to(DEV), [t_pad] * 7, torch.zeros(7, dtype=torch.int64, device=DEV))
    index = torch.tensor([0, 6, 3, 3, 1, 5, 2, 4, 0])
    time_bands = [(t0, tw) for t0 in (0, 1, 2, 3, 5, t_pad - 3, t_pad - 1, t_pad, -2) for tw in (0, 1, 2, 3, 4, 5, 9)]
    freq_bands = [(n_mels - 2, 5), (n_mels // 2, 0), (-1, 3), (0, 1)]   # across the top row, none, from below row 0, plain
    assert len(time_bands) == 63
    for call in range(7):
        tm = torch.tensor(time_bands[call * 9:call * 9 + 9], dtype=torch.int32)
        fm = torch.tensor([freq_bands[(b + call) % 4] for b in range(9)], dtype=torch.int32)
        want = host[index].clone()
        for b in range(9):
            _zero_band(want[b], 1, int(tm[b, 0]), int(tm[b, 1]), t_pad)
            _zero_band(want[b], 0, int(fm[b, 0]), int(fm[b, 1]), n_mels)
        assert torch.equal(store.gather(index.to(DEV), tm, fm).cpu(), want), call
    assert torch.equal(store.gather(index.to(DEV)).cpu(), host[index])
    ops.check_status()
    bad = index.clone()
    bad[2], bad[7] = -1, 7
    out = store.gather(bad.to(DEV)).cpu()
    with pytest.raises(_native.SirError):
        ops.check_status()
    ops.check_status()                                                  # reported once
    want = host[bad.clamp(0, 6)].clone()
    want[2], want[7] = 0.0, 0.0
    assert torch.equal(out, want)


# ---- h. mix beyond one pass of the grid ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 64, 260), (2, 64, 2052)])
def test_mix_long_rows_vs_float64(shape):
    """The two bounds of tests/test_recipe_gpu.py::test_mix_features_vs_float64, at rows of more than 16 x 256 float4."""
    bsz = shape[0]
    assert shape[1] * shape[2] // 4 > 4096
    g = torch.Generator().manual_seed(shape[2])
    x = torch.randn(shape, generator=g) * 4.0
    perm = torch.roll(torch.arange(bsz), 1)
    r = float(torch.rand(1, generator=g))
    for lam in ([[1.0, 0.0, 0.5], [r, 1.0, 0.5]] if bsz == 3 else [[1.0, 0.0], [0.5, r]]):
        lam = torch.tensor(lam)
        out = train_ops.mix_features(x.to(DEV), perm.to(DEV), lam.to(DEV)).cpu()
        om32 = 1.0 - lam
        l, om = lam.double().view(-1, 1, 1), om32.double().view(-1, 1, 1)
        a, b = x.double(), x.double()[perm]
        bound = 2 * U * ((l * a).abs() + (om * b).abs())
        err = (out.double() - recipe_ref.mix(x, perm, lam, complement=om32)).abs()
        delta = (om - (1.0 - l)).abs()
        err_def = (out.double() - recipe_ref.mix(x, perm, lam)).abs()
        bound_def = 2 * U * ((l * a).abs() + ((1.0 - l) * b).abs()) + delta * b.abs()
        print(f"mix {shape} lam {lam.tolist()}: max err / bound {(err / bound.clamp(min=1e-300)).max().item():.3f}, against the "
              f"real-number complement {(err_def / bound_def.clamp(min=1e-300)).max().item():.3f}")
        assert (err <= bound).all()
        assert (err_def <= bound_def).all()
        for row in range(bsz):
            if float(lam[row]) == 1.0:
                assert torch.equal(_bits(out[row]), _bits(x[row])), row
    ops.check_status()
