"""GPU parity of the general feature path (every front-end but n_fft 1024 / hop 512 / win_length 1024) against the float32
reference of tests/frontend_cfg_ref.py, and of the rest of the handle on such a front-end.

Tolerance: the project's feature tolerance |a - b| <= 1e-4 * max(1, |b|) (tests/test_features_gpu.py, BASELINE.json), on the dB
values and on the normalised output, every element.  The float32 reference itself stays within 1e-5 of float64 under that measure
on these signals (tests/test_frontend_cfg_host.py checks it at every configuration and length used here).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import frontend_cfg_ref as ref
from oracle import model_ref
from sir_amd import _native, featurizer, synth
from sir_amd.models.models import CNNAudioGRU

pytestmark = pytest.mark.gpu

TOL = 1e-4
DEV = "cuda"
CONFIGS = [(512, 160, 400), (256, 64, 256), (1024, 256, 1024), (1024, 512, 800), (512, 512, 512), (512, 129, 400)]
T_PAD = 48


def _close(a, b, tol=TOL):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))


def case_lengths(n_fft, hop):
    """n_fft/2 (zero row), n_fft/2 + 1, below n_fft (both reflections in one frame), a multiple of the hop, a multiple plus
    hop - 1, 38 frames (< T_PAD, not a multiple of the 16 frames of a round) and 71 frames (> T_PAD, a second 64-frame tile)."""
    return [n_fft // 2, n_fft // 2 + 1, n_fft - 37, 20 * hop, 20 * hop + hop - 1, 37 * hop + 5, 70 * hop + 3]


def _run(cfg, waves, t_pad=T_PAD, dtype=torch.float32, **kw):
    fz = featurizer.get_featurizer(16000, 64, *cfg)
    lengths = [int(w.numel()) for w in waves]
    batch = torch.zeros(len(waves), max(lengths), dtype=dtype)
    for i, w in enumerate(waves):
        batch[i, : w.numel()] = w.to(dtype)
    db = torch.full((len(waves), 64, t_pad), float("nan"), device=DEV)
    out = torch.full((len(waves), 64, t_pad), float("nan"), device=DEV)
    fz(batch.to(DEV), torch.tensor(lengths, dtype=torch.int32, device=DEV), t_pad=t_pad, db_out=db, out=out, **kw)
    torch.cuda.synchronize()
    return out.cpu(), db.cpu()


def _case_waves(n_fft, hop, seed=5):
    lengths = case_lengths(n_fft, hop)
    clips = ref.chirp_clips(len(lengths), max(lengths), seed)
    return [clips[i, :n] for i, n in enumerate(lengths)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "n%d_h%d_w%d" % c)
def test_parity_per_configuration(cfg):
    n_fft, hop, win = cfg
    waves = _case_waves(n_fft, hop)
    out, db = _run(cfg, waves)
    ref_out, ref_db = ref.batch_f32(waves, n_fft, hop, win, T_PAD)
    for i, w in enumerate(waves):
        t = min(ref.num_frames(w.numel(), n_fft, hop), T_PAD)
        derr = np.abs(db[i].numpy() - ref_db[i].numpy()).max()
        oerr = np.abs(out[i].numpy() - ref_out[i].numpy()).max()
        print(f"cfg {cfg} clip {i} L {w.numel()} frames {t}: max |db diff| {derr:.3e}, max |out diff| {oerr:.3e}")
        assert _close(db[i], ref_db[i]).all(), (cfg, i, derr)
        assert _close(out[i], ref_out[i]).all(), (cfg, i, oerr)
        assert (out[i, :, t:] == 0).all() and (db[i, :, t:] == 0).all(), (cfg, i)      # exact zeros behind the clip
    assert (out[0] == 0).all() and (db[0] == 0).all()                                  # L = n_fft / 2: zero row
    if cfg == (256, 64, 256):                          # the filter without a bin: exactly -100 dB wherever a frame exists
        fb = featurizer.htk_mel_fbanks(129, 0.0, 8000.0, 64, 16000)
        empty = [j for j in range(64) if not (fb[:, j] != 0).any()]
        assert empty, "n_fft 256 with 64 mel bands is expected to leave a filter without a bin"
        for j in empty:
            assert (db[6, j, :T_PAD] == -100.0).all()


def test_every_other_frame_is_the_shipped_kernels_frame():
    """(1024, 256, 1024) frames 0, 2, 4, ... of db_out are frames 0, 1, 2, ... of the default handle's, edge frames included."""
    waves = _case_waves(1024, 512, seed=6)[1:]                     # lengths 513 ... 70 * 512 + 3
    t_def = 1 + max(w.numel() for w in waves) // 512
    _, db_def = _run((1024, 512, 1024), waves, t_pad=t_def)
    _, db_gen = _run((1024, 256, 1024), waves, t_pad=2 * t_def)
    for i, w in enumerate(waves):
        t = 1 + w.numel() // 512
        a, b = db_gen[i, :, 0:2 * t:2], db_def[i, :, :t]
        assert a.shape == b.shape
        assert _close(a, b).all(), (i, np.abs(a.numpy() - b.numpy()).max())


@pytest.mark.parametrize("cfg", [(512, 129, 400), (512, 160, 400)], ids=lambda c: "n%d_h%d_w%d" % c)
def test_augmentation_and_int16(cfg):
    n_fft, hop, win = cfg
    w = ref.chirp_clips(4, 6000, seed=11)
    t_pad = 1 + 6000 // hop + 3
    base, base_db = _run(cfg, list(w), t_pad=t_pad)
    # PCM16 input = the float input s / 32768
    w16 = synth.to_int16(w)
    out16, db16 = _run(cfg, list(w16), t_pad=t_pad, dtype=torch.int16)
    r_out, r_db = ref.batch_f32(list(w16.float() / 32768.0), n_fft, hop, win, t_pad)
    assert _close(db16, r_db).all() and _close(out16, r_out).all()
    outf, _ = _run(cfg, list(w16.float() / 32768.0), t_pad=t_pad)
    assert _close(out16, outf).all()
    # an odd row stride moves every second row off the sample-pair boundary: same values
    odd = torch.zeros(4, 6001, dtype=torch.int16)
    odd[:, :6000] = w16
    fz = featurizer.get_featurizer(16000, 64, *cfg)
    out_odd = fz(odd.to(DEV)[:, :6000], t_pad=t_pad).cpu()
    assert _close(out_odd, out16, 2e-5).all()
    # device time shift = host-shifted clip (the bound of test_time_shift_matches_host_shift)
    shifts = [0, 333, -450, 1999]
    host = []
    for x, s in zip(w, shifts):
        y = torch.zeros_like(x)
        if s >= 0:
            y[s:] = x[: x.numel() - s]
        else:
            y[: x.numel() + s] = x[-s:]
        host.append(y)
    out_host, _ = _run(cfg, host, t_pad=t_pad)
    out_dev, _ = _run(cfg, list(w), t_pad=t_pad, shift=torch.tensor(shifts, dtype=torch.int32))
    assert (out_host - out_dev).abs().max().item() <= 2e-5
    # SpecAugment bands: exact zeros, the rest unchanged
    tm = torch.tensor([[10, 15], [0, 0], [3, 1], [0, 0]], dtype=torch.int32)
    fm = torch.tensor([[0, 0], [50, 10], [0, 4], [0, 0]], dtype=torch.int32)
    out, db = _run(cfg, list(w), t_pad=t_pad, time_mask=tm, freq_mask=fm)
    exp = base.clone()
    exp[0, :, 10:25] = 0
    exp[1, 50:60, :] = 0
    exp[2, :, 3:4] = 0
    exp[2, 0:4, :] = 0
    assert torch.equal(out, exp) and torch.equal(db, base_db)


@pytest.mark.parametrize("cfg", [(512, 129, 400), (512, 160, 400)], ids=lambda c: "n%d_h%d_w%d" % c)
def test_silence_and_noise_level(cfg):
    """Digital silence: -100 dB in every frame and a zero output, as the reference gives.  sigma * N(0, 1) on silence:
    E|X[k]|^2 = sigma^2 * sum(w^2) = sigma^2 * 0.375 * win_length per bin, so the frame-mean mel POWER of a filter is that times
    the filter's weight sum -- within 1.5 dB (the mean of >= 150 independent-frame equivalents of an exponential variable has a
    relative deviation of <= 8 %: 1.5 dB is four of those) -- and the frame-mean of the dB values sits below the dB of the mean
    (Jensen) by at most the 2.51 dB of a single exponential bin plus its own sampling error (5.6 dB / sqrt(150) = 0.45 dB: -5)."""
    n_fft, hop, win = cfg
    n = 64000
    t = 1 + n // hop
    sig = 0.01
    out, db = _run(cfg, [torch.zeros(n)] * 2, t_pad=t, noise_sigma=torch.tensor([sig, 0.0]), noise_seed=99)
    assert (db[1] == -100.0).all() and (out[1] == 0).all()
    r_out, r_db = ref.batch_f32([torch.zeros(n)], n_fft, hop, win, t)
    assert torch.equal(db[1], r_db[0]) and torch.equal(out[1], r_out[0])
    fb = featurizer.htk_mel_fbanks(n_fft // 2 + 1, 0.0, 8000.0, 64, 16000)
    expect = 10 * np.log10(sig * sig * 0.375 * win * fb.sum(0).double().numpy())
    inner = db[0, :, 4:t - 4].double().numpy()                     # frames clear of the reflected edges
    mean_power_db = 10 * np.log10(np.mean(10.0 ** (inner / 10.0), axis=1))
    assert np.all(np.abs(mean_power_db - expect) < 1.5), mean_power_db - expect
    mean_db = inner.mean(1)
    assert np.all(mean_db < expect + 0.5) and np.all(mean_db > expect - 5.0), mean_db - expect


def test_statistics_reproducibility_and_row_independence():
    cfg = (512, 160, 400)
    lengths = [257, 3000, 4799, 4800, 7013, 10240, 11000, 11359]
    clips = ref.chirp_clips(len(lengths), max(lengths), seed=21)
    waves = [clips[i, :n] for i, n in enumerate(lengths)]
    t_pad = 1 + max(lengths) // 160
    out, db = _run(cfg, waves, t_pad=t_pad)
    for i, n in enumerate(lengths):
        t = 1 + n // 160
        valid = out[i, :, :t].reshape(-1).double()
        assert abs(valid.mean().item()) < 1e-4 and abs(valid.std(unbiased=True).item() - 1.0) < 1e-4, (i, n)
        assert (out[i, :, t:] == 0).all()
    out2, db2 = _run(cfg, waves, t_pad=t_pad)
    assert torch.equal(out, out2) and torch.equal(db, db2)           # bit-identical from run to run
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    out_p, db_p = _run(cfg, [waves[i] for i in perm], t_pad=t_pad)   # another position, other neighbours, another max_len share
    assert torch.equal(out_p, out[perm]) and torch.equal(db_p, db[perm])
    out_1, _ = _run(cfg, [waves[4]], t_pad=t_pad)                     # alone: max_len (and the slab's row stride) differ
    assert torch.equal(out_1[0], out[4])
    # statistics over ALL frames although only t_pad are stored
    out_t, _ = _run(cfg, waves, t_pad=40)
    assert torch.equal(out_t, out[:, :, :40])


def test_rest_of_the_handle(monkeypatch):
    from sir_amd import ops
    fz_def = featurizer.get_featurizer()
    fz = featurizer.get_featurizer(16000, 64, 512, 160, 400)
    assert fz.num_frames(48000) == 301
    # sir_resample: the same bits on both handles
    w = ref.chirp_clips(3, 4410, seed=31).to(DEV)
    a, la = fz_def.resample(w, 44100, 16000)
    b, lb = fz.resample(w, 44100, 16000)
    assert torch.equal(a, b) and torch.equal(la, lb)
    # sir_model_infer: the same bits on both handles
    sd = synth.synth_state_dict(31, seed=0)
    x = synth.synth_features(3, 40, seed=7).to(DEV)

    def logits(handle_owner):
        m = CNNAudioGRU(31)
        m.load_state_dict(sd)
        m = m.to(DEV).eval()
        monkeypatch.setattr(ops, "get_featurizer", lambda *a, **k: handle_owner)
        lg, am = m.predict(x)
        torch.cuda.synchronize()
        return lg.cpu(), am.cpu()
    lg_def, am_def = logits(fz_def)
    lg_gen, am_gen = logits(fz)
    monkeypatch.undo()
    assert torch.equal(lg_def, lg_gen) and torch.equal(am_def, am_gen)
    # sir_features_bwd: SIR_EUNSUPPORTED, nothing written
    wave = ref.chirp_clips(2, 3000, seed=32).to(DEV)
    t_pad = 1 + 3000 // 160
    dbt = torch.empty(2, 64, t_pad, device=DEV)
    fz(wave, t_pad=t_pad, db_out=dbt)
    dwave = torch.full((2, 3000), 7.0, device=DEV)
    with pytest.raises(_native.SirError, match="default front-end only") as ei:
        fz.features_bwd(wave, None, dbt, torch.ones_like(dbt), t_pad=t_pad, out=dwave)
    assert f"code {_native.SIR_EUNSUPPORTED}" in str(ei.value)
    torch.cuda.synchronize()
    assert (dwave == 7.0).all()
    with pytest.raises(_native.SirError, match="default front-end only"):
        fz.differentiable(wave.clone().requires_grad_(True), t_pad=t_pad)
    # too small a workspace: SIR_ENOMEM, nothing launched
    lib = _native.lib()
    need = lib.sir_features_workspace_bytes(fz.handle, 2, 3000)
    assert need >= 2 * 64 * t_pad * 4
    assert lib.sir_features_workspace_bytes(fz_def.handle, 2, 3000) == 256
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    lens = torch.full((2,), 3000, dtype=torch.int32, device=DEV)
    outt = torch.full((2, 64, t_pad), 5.0, device=DEV)
    rc = lib.sir_features_fwd(fz.handle, wave.data_ptr(), _native.WAVE_F32, wave.stride(0), lens.data_ptr(), 2, 3000,
                              outt.data_ptr(), t_pad, None, ws.data_ptr(), need - 1, None, _native.current_stream_ptr())
    torch.cuda.synchronize()
    assert rc == -2 and (outt == 5.0).all()


@pytest.mark.parametrize("n_fft,hop,win", [(2048, 512, 0), (384, 96, 0), (512, 0, 0), (512, 513, 0), (512, 31, 0), (1024, 63, 0),
                                           (256, 15, 0), (512, 160, 513), (1024, 512, 1025), (512, 160, -1)])
def test_unsupported_front_ends_are_refused(n_fft, hop, win):
    cfg = _native.FeatureConfig(16000, n_fft, hop, 64, 0.0, 8000.0, None, None)
    h = C.c_void_p()
    rc = _native.lib().sir_create_ex(C.byref(cfg), win, C.byref(h))
    assert rc == _native.SIR_EUNSUPPORTED and not h.value
    msg = _native.lib().sir_last_error().decode()
    assert "256, 512, 1024" in msg and "win_length" in msg
    if win == 0:
        assert _native.lib().sir_create(C.byref(cfg), C.byref(h)) == _native.SIR_EUNSUPPORTED


def test_library_window_and_filterbank_match_torchs():
    """cfg->window / cfg->mel_fb NULL: the library's own periodic Hann of win_length and HTK bank, computed in double."""
    cfg = _native.FeatureConfig(16000, 512, 160, 64, 0.0, 8000.0, None, None)
    h = C.c_void_p()
    lib = _native.lib()
    _native.check(lib.sir_create_ex(C.byref(cfg), 400, C.byref(h)), "sir_create_ex")
    try:
        w = ref.chirp_clips(2, 4000, seed=41)
        t_pad = 1 + 4000 // 160
        wave = w.to(DEV)
        lens = torch.full((2,), 4000, dtype=torch.int32, device=DEV)
        need = lib.sir_features_workspace_bytes(h, 2, 4000)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        out = torch.empty(2, 64, t_pad, device=DEV)
        rc = lib.sir_features_fwd(h, wave.data_ptr(), _native.WAVE_F32, wave.stride(0), lens.data_ptr(), 2, 4000,
                                  out.data_ptr(), t_pad, None, ws.data_ptr(), need, None, _native.current_stream_ptr())
        _native.check(rc, "sir_features_fwd")
        torch.cuda.synchronize()
        r_out, _ = ref.batch_f32(list(w), 512, 160, 400, t_pad)
        assert _close(out.cpu(), r_out).all()
    finally:
        lib.sir_destroy(h)


def test_end_to_end_at_hop_160():
    """CNNAudioGRU scored on 3 s clips at 25 ms / 10 ms (301 frames, t_pad 304) against the float64 model oracle fed the same
    features: identical argmax, logits within the 1e-4 * max(1, |b|) of the model tests."""
    fz = featurizer.get_featurizer(16000, 64, 512, 160, 400)
    wave = synth.synth_clips(4, 48000, seed=77)
    feats = fz(wave.to(DEV), t_pad=304)
    sd = synth.synth_state_dict(31, seed=0)
    m = CNNAudioGRU(31)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    logits, pred = m.predict(feats)
    torch.cuda.synchronize()
    r_feats, _ = ref.batch_f32(list(wave), 512, 160, 400, 304)
    assert _close(feats.cpu(), r_feats).all()
    with torch.no_grad():
        r_logits = model_ref.forward(sd, feats.cpu())
    err = ((logits.cpu().double() - r_logits.double()).abs() / r_logits.double().abs().clamp(min=1.0)).max().item()
    print("hop-160 end to end: logits max rel-abs error", err)
    assert err <= 1e-4
    assert torch.equal(pred.cpu(), r_logits.argmax(1))


def test_predict_from_a_file_at_hop_160(tmp_path):
    """scripts/predict_frontend.predict: a PCM16 file scored at 512 / 160 / 400 with 304 frames gives the label the float64 model
    oracle gives on the reference's features of the same samples."""
    from sir_amd.scripts import predict_frontend as pf
    from sir_amd.scripts.utils import wav_io
    w16 = synth.to_int16(synth.synth_clips(1, 48000, seed=78))[0]
    path = str(tmp_path / "clip.wav")
    wav_io.write_wav_pcm16(path, w16, 16000)
    sd = synth.synth_state_dict(31, seed=0)
    m = CNNAudioGRU(31)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    label_map = {f"intent_{i}": i for i in range(31)}
    res = pf.predict(m, path, label_map, torch.device(DEV), pad_to=304, frontend={"n_fft": 512, "hop_length": 160, "win_length": 400})
    r_feats, _ = ref.batch_f32([w16.float() / 32768.0], 512, 160, 400, 304)
    with torch.no_grad():
        r_logits = model_ref.forward(sd, r_feats)
    assert res is not None and res["predicted_label"] == f"intent_{int(r_logits.argmax(1))}"
    assert res["top_predictions"][0]["label"] == res["predicted_label"] and 0.0 < res["confidence"] <= 1.0


def test_batch_pipeline_and_prefetcher_on_a_general_front_end():
    """The slots of a BatchPipeline run batches of ONE featurizer on several streams at once, and on a general front-end the feature
    workspace is the live dB slab between the two launches: every stream has its own.  Features, logits and argmax of batches of
    different lengths are bit-identical to the in-line call for 1, 2 and 3 slots; so are the FeaturePrefetcher's buffers."""
    from sir_amd.pipeline import BatchPipeline, FeaturePrefetcher
    fe = (512, 160, 400)
    fz = featurizer.get_featurizer(16000, 64, *fe)
    m = CNNAudioGRU(31)
    m.load_state_dict(synth.synth_state_dict(31, seed=0))
    m = m.to(DEV).eval()
    waves = [synth.synth_clips(32, 20000 + 1600 * i, seed=400 + i).to(DEV) for i in range(8)]
    t_pad = 1 + 31200 // 160 + 1                                   # 196 frames + padding to a multiple of 4
    want = []
    for w in waves:
        f = fz(w, t_pad=t_pad).clone()
        want.append((f, *m.predict(f)))
    torch.cuda.synchronize()
    for n in (1, 2, 3):
        pipe = BatchPipeline(m, n_streams=n, frontend=fe)
        assert pipe.featurizer is fz
        outs = [torch.empty(32, 64, t_pad, device=DEV) for _ in waves]
        res = []
        for i, w in enumerate(waves):
            f = pipe.features(i, w, None, t_pad=t_pad, out=outs[i])
            res.append((f, *pipe.infer(i, f)))
        pipe.synchronize()
        for i, ((f0, l0, a0), (f1, l1, a1)) in enumerate(zip(want, res)):
            assert torch.equal(f0, f1), (n, i)
            assert torch.equal(l0, l1) and torch.equal(a0, a1), (n, i)
    pre = FeaturePrefetcher(t_pad=t_pad, frontend=fe)
    assert (pre.fz.n_fft, pre.fz.hop_length, pre.fz.win_length) == fe
    pre.submit(waves[0])
    for i in range(len(waves)):
        if i + 1 < len(waves):
            pre.submit(waves[i + 1])                                # one batch ahead, on the side stream
        got = pre.get().clone()
        pre.release()
        torch.cuda.synchronize()
        assert torch.equal(got, want[i][0]), i


def test_a_bank_too_large_for_the_general_kernels_lds_is_refused_at_create():
    """64 filters of 50 taps = 3200 taps pass sir_create's 4096-tap rule, but at n_fft 1024 the general frames kernel would need
    more than the 160 KB of LDS: the handle is refused when it is created, not at its first launch.  The default front-end
    (another kernel, smaller buffers) still takes the same bank."""
    fb = torch.zeros(513, 64)
    for j in range(64):
        fb[7 * j: 7 * j + 50, j] = 1.0
    lib = _native.lib()
    h = C.c_void_p()
    cfg = _native.FeatureConfig(16000, 1024, 256, 64, 0.0, 8000.0, None, fb.data_ptr())
    assert lib.sir_create_ex(C.byref(cfg), 0, C.byref(h)) == _native.SIR_EUNSUPPORTED and not h.value
    assert "LDS" in lib.sir_last_error().decode()
    cfg = _native.FeatureConfig(16000, 1024, 512, 64, 0.0, 8000.0, None, fb.data_ptr())
    assert lib.sir_create_ex(C.byref(cfg), 0, C.byref(h)) == _native.SIR_OK
    lib.sir_destroy(h)
