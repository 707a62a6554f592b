"""GPU: sir_wave_perturb (HipFeaturizer.perturb) against the float64 contract of tests/wave_perturb_ref.py.

WSOLA's argmin is discontinuous, so each pass is rebuilt in float64 from the offsets the kernel chose (the offsets_out
test hook): at every segment the kernel's offset must be a float64 minimum up to float32 rounding, it must BE the float64
argmin almost everywhere, and the output rebuilt from those offsets must match the kernel's samples."""
import random

import numpy as np
import pytest
import torch

import wave_perturb_ref as ref
from oracle import features_ref
from sir_amd import ops, synth
from sir_amd.scripts import augment as aug

pytestmark = pytest.mark.gpu

SR = 16000
H = 1120
MAX_SEG = 64
LENGTHS = [48000, 0, 300, 1312, 5000, 47999, 48000, 30000]


@pytest.fixture(scope="module")
def fz():
    from sir_amd.featurizer import get_featurizer
    return get_featurizer()


def _batch(dtype):
    x = synth.synth_clips(len(LENGTHS), 48000, seed=77)
    if dtype == torch.int16:
        x = (x * 32767.0).round().to(torch.int16)
    for b, n in enumerate(LENGTHS):
        x[b, n:] = 0
    return x


def _host_f64(x, b):
    row = x[b, :LENGTHS[b]]
    return row.double().numpy() / (32768.0 if x.dtype == torch.int16 else 1.0)


class _Tally:
    def __init__(self):
        self.segments = self.argmin_hits = 0

    def check_pass(self, kernel_offs, costs):
        """kernel_offs: offsets of one pass (-1 beyond its segments); costs: float64 candidate costs per segment j >= 1."""
        used = kernel_offs[kernel_offs >= 0]
        assert len(used) == len(costs) + (1 if len(used) else 0)
        for j, c in enumerate(costs, start=1):
            o = int(used[j])
            assert 0 <= o < len(c)
            assert c[o] <= c.min() * (1 + 1e-4) + 1e-6, (j, o, c[o], c.min())
            self.segments += 1
            self.argmin_hits += int(o == int(np.argmin(c)))

    def check_rate(self):
        assert self.segments > 100 and self.argmin_hits >= 0.99 * self.segments, (self.argmin_hits, self.segments)


def _run(fz, x, **kw):
    offs = torch.full((x.shape[0], 2, MAX_SEG), 7, dtype=torch.int32, device="cuda")
    lens = torch.tensor(LENGTHS, dtype=torch.int32, device="cuda")
    dev = {k: (v.cuda() if v is not None else None) for k, v in kw.items()}
    out, out_len = fz.perturb(x.cuda(), lens, offsets_out=offs, **dev)
    torch.cuda.synchronize()
    ops.check_status()
    return out.cpu(), out_len.cpu(), offs.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
def test_tempo_matches_float64_contract(fz, dtype):
    x = _batch(dtype)
    tally = _Tally()
    rng = np.random.default_rng(3)
    factors = [[f] * len(LENGTHS) for f in (0.85, 0.9, 1.1, 1.15)] + [rng.uniform(0.85, 1.15, len(LENGTHS)).tolist()]
    for fs in factors:
        tempo = torch.tensor(fs, dtype=torch.float32)
        out, out_len, offs = _run(fz, x, tempo=tempo)
        assert (offs[:, 0] == -1).all()
        for b, n in enumerate(LENGTHS):
            f = float(tempo[b])
            want_len = ref.out_len(n, f)
            assert int(out_len[b]) == want_len == aug.perturbed_out_len(n, f)
            xb = _host_f64(x, b)
            y, used, costs = ref.tempo(xb, f, offsets=offs[b, 1])
            assert len(used) == int((offs[b, 1] >= 0).sum()) == -(-want_len // H)
            tally.check_pass(offs[b, 1], costs)
            scale = max(np.abs(xb).max() if n else 0.0, 1e-30)
            got = out[b].double().numpy()
            assert np.abs(got[:want_len] - y).max(initial=0.0) <= 1e-6 * scale, (b, f)
            assert (got[want_len:] == 0).all()
    tally.check_rate()


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
def test_pitch_matches_float64_contract(fz, dtype):
    x = _batch(dtype)
    tally = _Tally()
    for c in (-200.0, -37.5, 150.0, 200.0):
        cents = torch.full((len(LENGTHS),), c, dtype=torch.float32)
        out, out_len, offs = _run(fz, x, pitch_cents=cents)
        assert (offs[:, 1] == -1).all()
        d = 2.0 ** (c / 1200.0)
        for b, n in enumerate(LENGTHS):
            assert int(out_len[b]) == n
            xb = _host_f64(x, b)
            s, used, costs = ref.tempo(xb, 1.0 / d, offsets=offs[b, 0])
            assert len(s) == ref.out_len(n, 1.0 / d) and len(used) == int((offs[b, 0] >= 0).sum())
            tally.check_pass(offs[b, 0], costs)
            y = ref.resample_frac(s, d, n)
            scale = max(np.abs(xb).max() if n else 0.0, 1e-30)
            got = out[b].double().numpy()
            assert np.abs(got[:n] - y).max(initial=0.0) <= 2e-6 * scale, (b, c, np.abs(got[:n] - y).max() / scale)
            assert (got[n:] == 0).all()
    tally.check_rate()


def _chain_params(seed=5):
    shift, cents, tempo, sigma = aug.draw_batch_params_full(LENGTHS * 2, 1.0, random.Random(seed))
    # make sure every combination is present: rows 0-3 none / pitch / speed / both, rest as drawn
    cents[:4] = torch.tensor([0.0, 120.0, 0.0, -150.0])
    tempo[:4] = torch.tensor([1.0, 1.0, 0.9, 1.12])
    shift[:4] = torch.tensor([2000, -500, 0, 700], dtype=torch.int32)
    return shift, cents, tempo


def test_chain_identity_rows_and_determinism(fz):
    x = torch.cat([_batch(torch.float32)] * 2)
    lens = torch.tensor(LENGTHS * 2, dtype=torch.int32)
    shift, cents, tempo = _chain_params()
    outs = []
    for _ in range(2):
        offs = torch.full((x.shape[0], 2, MAX_SEG), 7, dtype=torch.int32, device="cuda")
        out, out_len = fz.perturb(x.cuda(), lens.cuda(), shift=shift.cuda(), pitch_cents=cents.cuda(), tempo=tempo.cuda(),
                                  offsets_out=offs)
        torch.cuda.synchronize()
        ops.check_status()
        outs.append((out.cpu(), out_len.cpu(), offs.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    out, out_len, offs = outs[0]
    for b in range(x.shape[0]):
        n = int(lens[b])
        assert int(out_len[b]) == min(aug.perturbed_out_len(n, float(tempo[b])), out.shape[1])
        if cents[b] == 0 and tempo[b] == 1:
            xs = torch.from_numpy(ref.shifted(x[b, :n].double().numpy(), int(shift[b]))).float()
            assert torch.equal(out[b, :n], xs) and (out[b, n:] == 0).all(), b
            assert (offs[b] == -1).all()
    # the combined row 3 (pitch then speed, shifted) against the float64 chain rebuilt from the kernel's offsets
    n = LENGTHS[3]
    xs = ref.shifted(x[3, :n].double().numpy(), int(shift[3]))
    y, _, _, _ = ref.pitch(xs, float(cents[3]), offsets=offs[3, 0].numpy())
    z, _, costs = ref.tempo(y, float(tempo[3]), offsets=offs[3, 1].numpy())
    m = int(out_len[3])
    assert m == len(z) and np.abs(out[3, :m].double().numpy() - z).max() <= 4e-6 * np.abs(xs).max()


def test_out_of_range_factor_is_reported(fz):
    from sir_amd import _native
    x = _batch(torch.float32).cuda()
    lens = torch.tensor(LENGTHS, dtype=torch.int32, device="cuda")
    tempo = torch.ones(len(LENGTHS))
    tempo[2] = 3.0
    out, out_len = fz.perturb(x, lens, tempo=tempo.cuda())
    with pytest.raises(_native.SirError):
        ops.check_status()
    assert int(out_len[2]) == 0 and (out[2] == 0).all() and int(out_len[0]) == 48000
    ops.check_status()                                           # the flag was cleared by the check that raised


def test_perturbed_features_match_oracle(fz):
    x = _batch(torch.float32)
    cents = torch.tensor([150.0, 0.0, -120.0, 0.0, 90.0, -200.0, 0.0, 37.5])
    tempo = torch.tensor([1.0, 0.88, 1.1, 1.0, 0.95, 1.15, 1.05, 0.85])
    offs = torch.full((len(LENGTHS), 2, MAX_SEG), 7, dtype=torch.int32, device="cuda")
    lens = torch.tensor(LENGTHS, dtype=torch.int32, device="cuda")
    wave, wlen = fz.perturb(x.cuda(), lens, pitch_cents=cents.cuda(), tempo=tempo.cuda(), offsets_out=offs)
    feats = fz(wave, wlen, t_pad=200).cpu()
    ops.check_status()
    offs = offs.cpu().numpy()
    rebuilt = torch.zeros(wave.shape, dtype=torch.float32)
    wlen = wlen.cpu()
    for b, n in enumerate(LENGTHS):
        y = ref.pitch(_host_f64(x, b), float(cents[b]), offsets=offs[b, 0])[0]
        z = ref.tempo(y, float(tempo[b]), offsets=offs[b, 1])[0]
        assert len(z) == int(wlen[b])
        rebuilt[b, :len(z)] = torch.from_numpy(z).float()
    for b in range(len(LENGTHS)):
        f = features_ref.extract_features_f32(rebuilt[b, :int(wlen[b])])
        if f is None:                                            # <= 512 samples: the reference's zero spectrogram
            assert (feats[b] == 0).all(), b
            continue
        want = features_ref.pad_or_trim(f)
        err = ((feats[b] - want).abs() / want.abs().clamp(min=1.0)).max().item()
        assert err <= 1e-4, (b, err)


@pytest.mark.parametrize("reverb", [False, True], ids=["perturb", "perturb_reverb"])
def test_two_pipeline_slots_in_flight_keep_their_own_scratch(fz, reverb):
    """Two BatchPipeline slots run the wave stages of one featurizer at once, both with a pitch drawn (the perturb workspace is
    live across three launches) and, with ``reverb``, through ``reverb_mix`` too: each slot's features are bit for bit those
    of the same calls in line -- the same kernels on the same inputs --, and the two slot streams hold scratch buffers of
    their own.  Batch B is batch A with rows and parameters reversed, so a slot that read the other's rows would show."""
    from sir_amd.models.models import CNNAudioGRU
    from sir_amd.pipeline import BatchPipeline
    from sir_amd.sound_bank import SoundBank
    xa = torch.cat([_batch(torch.float32)] * 2).cuda()
    lens = torch.tensor(LENGTHS * 2, dtype=torch.int32, device="cuda")
    kwa = dict(zip(("shift", "pitch_cents", "tempo"), (p.cuda() for p in _chain_params())))
    mix = {}
    if reverb:                                                   # the bank of test_reverb_gpu.py::test_batch_pipeline_features
        mix["rir"] = SoundBank([synth.synthetic_rir(0.1, rng=np.random.default_rng(6))], kind="rir")
        kwa["rir_index"] = torch.tensor([0, -1, 0, 0] * 4, dtype=torch.int32, device="cuda")
    batches = [(xa, lens, kwa), (xa.flip(0).contiguous(), lens.flip(0).contiguous(), {k: v.flip(0).contiguous() for k, v in kwa.items()})]
    want = []
    for x, n, kw in batches:
        w, wn = fz.perturb(x, n, shift=kw["shift"], pitch_cents=kw["pitch_cents"], tempo=kw["tempo"])
        if reverb:
            w = fz.reverb_mix(w, wn, rir_index=kw["rir_index"], **mix)
        want.append(fz(w, wn, t_pad=200))
    torch.cuda.synchronize()
    ops.check_status()
    pipe = BatchPipeline(CNNAudioGRU(num_classes=31).cuda().eval(), n_streams=2)
    assert pipe.featurizer is fz
    got = [pipe.features(i, x, n, t_pad=200, **kw, **mix) for i, (x, n, kw) in enumerate(batches)]
    pipe.synchronize()
    ops.check_status()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(want[0], want[1])
    slots = {st.cuda_stream for st in pipe.streams}
    spans = sorted((buf.data_ptr(), buf.data_ptr() + buf.numel()) for (_, st), buf in fz._scratch.buffers.items() if st in slots)
    assert len(slots) == 2 and len(spans) == 2 and spans[0][1] <= spans[1][0]


def test_train_with_pitch_speed_augment(tmp_path):
    import types
    from test_pipeline_gpu import _make_corpus, _write_splits
    from sir_amd.scripts import train as tr
    rows = _make_corpus(str(tmp_path / "wav"))
    csvs, lm = _write_splits(tmp_path, rows)
    cfg = {"batch_size": 8, "num_workers": 0, "num_labels": 31, "lr": 1e-3, "weight_decay": 1e-4, "epochs": 2,
           "early_stop_patience": 5, "augment_prob": 0.7, "use_feature_cache": False, "cache_dir": str(tmp_path / "nocache"),
           "save_path": str(tmp_path / "ckpt"), "pitch_speed_augment": True, "waveform_augment_prob": 1.0, "seed": 2}
    args = types.SimpleNamespace(train_csv=csvs["train"], val_csv=csvs["valid"], label_map=lm)
    losses = []
    orig = tr.train_epoch_waveforms

    def spy(*a, **k):
        loss = orig(*a, **k)
        losses.append(loss)
        return loss
    tr.train_epoch_waveforms = spy
    try:
        best = tr.train(args, cfg)
    finally:
        tr.train_epoch_waveforms = orig
    assert 0.0 <= best <= 1.0 and len(losses) == 2 and all(np.isfinite(losses))
    ops.check_status()
    lengths = [48000, 30000, 16000, 700]
    kw = tr.make_waveform_augment(dict(cfg, augment_prob=1.0), seed=2, epoch=0)(0, 4, lengths)
    assert set(kw) == {"shift", "pitch_cents", "tempo", "noise_sigma", "noise_seed", "time_mask", "freq_mask"}
    frames = [1 + aug.perturbed_out_len(n, f) // 512 for n, f in zip(lengths, kw["tempo"].tolist())]
    tm = kw["time_mask"]
    assert all(int(tm[b, 0]) + int(tm[b, 1]) <= max(frames[b], int(tm[b, 1])) for b in range(4))
