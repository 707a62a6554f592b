"""CPU: the reference of the general front-ends is sound (float32 against float64 at every configuration and length the GPU tests
use), the front-end keys are parsed once and reach every consumer, a feature cache of another front-end has another file name,
and the new entry point is declared and bound.  No device call is made."""
import json
import os
import re

import numpy as np
import pytest
import torch

import frontend_cfg_ref as ref
from sir_amd import _native
from sir_amd.frontend_config import DEFAULT, FrontEnd, as_frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(512, 160, 400), (256, 64, 256), (1024, 256, 1024), (1024, 512, 800), (512, 512, 512), (512, 129, 400)]


def _lengths(n_fft, hop):            # tests/test_frontend_cfg_gpu.py::case_lengths
    return [n_fft // 2, n_fft // 2 + 1, n_fft - 37, 20 * hop, 20 * hop + hop - 1, 37 * hop + 5, 70 * hop + 3]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "n%d_h%d_w%d" % c)
def test_float32_reference_is_close_to_float64(cfg):
    """Every element within 1e-5 under the feature measure |a - b| / max(1, |b|), a tenth of the kernel's tolerance: the reference's
    own float32 error cannot use that tolerance up.  (A float32 transform of n_fft points carries a relative error of about
    log2(n_fft) * 2^-24 = 6e-7 on a bin's power, 2.6e-6 dB, and a few times that on the weakest bins of a frame.)"""
    n_fft, hop, win = cfg
    lengths = _lengths(n_fft, hop)
    clips = ref.chirp_clips(len(lengths), max(lengths), seed=5)
    assert ref.features_f32(clips[0, :lengths[0]], n_fft, hop, win) is None        # n_fft / 2 samples: no reflect padding
    assert ref.features_f64(clips[0, :lengths[0]], n_fft, hop, win) is None
    for i, n in enumerate(lengths[1:], start=1):
        a = ref.features_f32(clips[i, :n], n_fft, hop, win)
        b = ref.features_f64(clips[i, :n].numpy(), n_fft, hop, win)
        assert a["db"].shape == b["db"].shape == (64, ref.num_frames(n, n_fft, hop))
        for k in ("db", "norm"):
            err = np.abs(a[k].double().numpy() - b[k]) / np.maximum(1.0, np.abs(b[k]))
            assert err.max() <= 1e-5, (cfg, n, k, err.max())


def test_reference_at_the_default_front_end_is_the_oracles():
    from oracle import features_ref
    x = ref.chirp_clips(1, 5000, seed=3)[0]
    a = ref.features_f32(x, 1024, 512, 1024)
    b = features_ref.extract_features_f32(x, stages=True)
    assert torch.equal(a["db"], b["db"]) and torch.equal(a["norm"], b["norm"])
    # (the oracle's float64 twin builds its filterbank in double, this one takes torchaudio's float32 table: weights differ by
    # float32 rounding, up to 5e-6 relative = 2e-5 dB on a filter of the 1024-point bank, over a standard deviation of >= 5 dB)
    assert np.abs(ref.features_f64(x.numpy(), 1024, 512)["norm"] - features_ref.extract_features_f64(x.numpy())).max() <= 1e-5


def test_n_fft_256_leaves_a_filter_without_a_bin():
    from sir_amd.featurizer import htk_mel_fbanks
    # torchaudio's float32 table against the float64 one: float32 rounding only -- band edges of up to 8000 Hz carry 2^-24 * 8000 =
    # 5e-4 Hz, over a narrowest band of 32 Hz: 1.5e-5 of a weight
    for n_freqs in (129, 257, 513):
        assert np.abs(htk_mel_fbanks(n_freqs, 0.0, 8000.0, 64, 16000).double().numpy() - ref.mel_fbank_f64(n_freqs)).max() <= 2e-5
    fb = htk_mel_fbanks(129, 0.0, 8000.0, 64, 16000)
    empty = [j for j in range(64) if not (fb[:, j] != 0).any()]
    assert len(empty) == 1
    x = ref.chirp_clips(1, 2000, seed=4)[0]
    assert (ref.features_f32(x, 256, 64)["db"][empty[0]] == -100.0).all()
    assert max(int((htk_mel_fbanks(513, 0.0, 8000.0, 64, 16000)[:, j] != 0).sum()) for j in range(64)) <= 42


def test_front_end_keys_and_defaults():
    assert FrontEnd.from_config({}) == FrontEnd.from_config(None) == DEFAULT == (1024, 512, 1024)
    assert DEFAULT.is_default and as_frontend(None) is DEFAULT
    fe = FrontEnd.from_config({"n_fft": 512, "hop_length": 160, "win_length": 400, "batch_size": 8})
    assert fe == (512, 160, 400) and not fe.is_default and fe.num_frames(48000) == 301 and fe.max_samples(304) == 304 * 160 - 1
    assert FrontEnd.from_config({"n_fft": 512}) == (512, 512, 512)                 # win_length defaults to n_fft, the hop stays 512
    assert FrontEnd.from_config({"hop_length": 256}) == (1024, 256, 1024)
    assert FrontEnd.from_config({"n_fft": 1024, "hop_length": 512, "win_length": None}).is_default
    assert not FrontEnd(1024, 512, 800).is_default
    assert as_frontend((512, 160)) == (512, 160, 512) and as_frontend({"n_fft": 256, "hop_length": 64}) == (256, 64, 256)
    assert as_frontend(fe) is fe
    for bad in ((2048, 512, None), (384, 96, None), (512, 0, None), (512, 513, None), (512, 31, None), (512, 160, 513), (512, 160, 0)):
        with pytest.raises(ValueError, match="256, 512, 1024"):
            FrontEnd(*bad)


def test_cache_file_name():
    assert DEFAULT.cache_name("train") == "train_features.pt"                      # today's name
    assert FrontEnd(1024, 512, 1024).cache_name("train") == "train_features.pt"
    assert FrontEnd(512, 160, 400).cache_name("train") == "train_features_n512_h160_w400.pt"
    assert FrontEnd(1024, 512, 800).cache_name("valid") == "valid_features_n1024_h512_w800.pt"
    names = {FrontEnd(*c).cache_name("x") for c in CONFIGS + [(1024, 512, 1024)]}
    assert len(names) == len(CONFIGS) + 1


def _bar_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_native, "lib", no_device)
    monkeypatch.setattr(_native, "require_hip", no_device)


class _FakeFeaturizer:
    device = torch.device("cpu")

    def __init__(self, args):
        self.args = args
        self.hop_length = args[3]

    def num_frames(self, n):
        return 1 + n // self.hop_length

    def __call__(self, wave, lens, t_pad):
        return torch.zeros(wave.shape[0], 64, t_pad)


def _record_featurizers(monkeypatch):
    from sir_amd.scripts import precompute_features
    made = []

    def fake(*args):
        made.append(args)
        return _FakeFeaturizer(args)
    monkeypatch.setattr(precompute_features, "get_featurizer", fake)
    return made


def test_extractor_passes_its_front_end_on(monkeypatch):
    from sir_amd.scripts.precompute_features import AudioFeatureExtractor
    _bar_device(monkeypatch)
    made = _record_featurizers(monkeypatch)
    ex = AudioFeatureExtractor(16000, 64, 512, 160, 400)
    assert (ex.n_fft, ex.hop_length, ex.win_length) == (512, 160, 400)
    ex._featurizer()
    AudioFeatureExtractor()._featurizer()
    AudioFeatureExtractor(16000, 64, 256, 64)._featurizer()
    assert made == [(16000, 64, 512, 160, 400), (16000, 64, 1024, 512, 1024), (16000, 64, 256, 64, 256)]
    # "clip too short" is judged by the extractor's own n_fft / 2
    lens = torch.tensor([256, 257, 600], dtype=torch.int32)
    monkeypatch.setattr(AudioFeatureExtractor, "waveforms_of_group", lambda self, d, c, sr, md: (torch.zeros(3, 600), lens))
    feats, frames, ok = ex._features_of_group([None] * 3, 1, 16000, 5.0)
    assert ok == [False, True, True] and frames == [2, 2, 4] and feats.shape == (3, 64, 4)
    _, frames, ok = AudioFeatureExtractor()._features_of_group([None] * 3, 1, 16000, 5.0)
    assert ok == [False, False, True] and frames == [1, 1, 2]


@pytest.fixture()
def split(tmp_path):
    csv = tmp_path / "train.csv"
    csv.write_text("path,label\n" + "".join(f"{tmp_path}/missing_{i}.wav,a\n" for i in range(3)))
    lm = tmp_path / "label_map.json"
    lm.write_text(json.dumps({"a": 0}))
    return str(csv), str(lm), tmp_path


def test_dataset_passes_its_front_end_on_and_keeps_caches_apart(split, monkeypatch):
    from sir_amd.scripts.dataset import FSCIntentDataset
    csv, lm, tmp = split
    _bar_device(monkeypatch)
    made = _record_featurizers(monkeypatch)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)               # no prefetch in the constructor
    cache = tmp / "cache"
    cache.mkdir()
    path0 = f"{tmp}/missing_0.wav"
    torch.save({path0: {"features": torch.ones(64, 5), "label": "a"}}, str(cache / "train_features.pt"))
    torch.save({path0: {"features": torch.full((64, 7), 2.0), "label": "a"}}, str(cache / "train_features_n512_h160_w400.pt"))
    ds = FSCIntentDataset(csv, lm, is_training=False, cache_dir=str(cache))
    assert ds.frontend.is_default and os.path.basename(ds.cache_file) == "train_features.pt"
    assert ds[0][0].shape == (64, 200) and (ds[0][0][:, :5] == 1).all()
    ds2 = FSCIntentDataset(csv, lm, is_training=False, cache_dir=str(cache), n_fft=512, hop_length=160, win_length=400,
                           mel_spec_length=304)
    assert os.path.basename(ds2.cache_file) == "train_features_n512_h160_w400.pt"
    assert ds2[0][0].shape == (64, 304) and (ds2[0][0][:, :7] == 2).all()       # never the default front-end's item
    ds3 = FSCIntentDataset(csv, lm, is_training=False, cache_dir=str(cache), n_fft=256, hop_length=64)
    assert not ds3.features_dict                                                  # no cache of this front-end: nothing is borrowed
    ds2._new_extractor()._featurizer()
    ds._new_extractor()._featurizer()
    assert made == [(16000, 64, 512, 160, 400), (16000, 64, 1024, 512, 1024)]
    with pytest.raises(ValueError):
        FSCIntentDataset(csv, lm, cache_dir=str(cache), n_fft=2048)


def test_frame_counts_take_the_front_ends_hop(monkeypatch):
    from sir_amd import waveform_store
    from sir_amd.scripts import augment, train
    assert waveform_store.frames_of([48000, 159, 160]) == [94, 1, 1]
    assert waveform_store.frames_of([48000, 159, 160], frontend=FrontEnd(512, 160, 400)) == [301, 1, 2]
    assert waveform_store.frames_of([48000], frontend={"hop_length": 256}) == [188]
    seen = []

    def draw(frames, prob, rng=None):
        seen.append(list(frames))
        return None, None
    monkeypatch.setattr(augment, "draw_spec_masks", draw)
    train.make_waveform_augment({"augment_prob": 1.0}, seed=1)(0, 2, [48000, 1000])
    train.make_waveform_augment({"augment_prob": 1.0, "n_fft": 512, "hop_length": 160, "win_length": 400}, seed=1)(0, 2, [48000, 1000])
    assert seen == [[94, 2], [301, 7]]


def test_pipeline_commands_carry_a_non_default_front_end():
    from sir_amd import run_pipeline
    base = run_pipeline.stage_commands("c.yaml", {}, "tr.csv", "va.csv", "te.csv", "lm.json")
    assert "--n_fft" not in base["precompute"]
    cmds = run_pipeline.stage_commands("c.yaml", {"n_fft": 512, "hop_length": 160, "win_length": 400}, "tr.csv", "va.csv", "te.csv",
                                       "lm.json")
    assert cmds["precompute"] == base["precompute"] + ["--n_fft", "512", "--hop_length", "160", "--win_length", "400"]
    assert cmds["train"] == base["train"] and cmds["evaluate"] == base["evaluate"]   # they read the keys from the config file


def test_differentiable_refuses_another_front_end_before_any_device_call(monkeypatch):
    from sir_amd import featurizer
    _bar_device(monkeypatch)
    monkeypatch.setattr(featurizer, "get_featurizer", _native.lib)
    fz = object.__new__(featurizer.HipFeaturizer)                # (no handle: creating one is a device call)
    fz.n_fft, fz.hop_length, fz.win_length, fz.n_mels, fz._h = 512, 160, 400, 64, None
    wave = torch.zeros(2, 4000)
    with pytest.raises(_native.SirError, match="default front-end only"):
        fz.differentiable(wave, t_pad=32)
    fz.n_fft, fz.hop_length, fz.win_length = 1024, 512, 800
    with pytest.raises(_native.SirError, match="default front-end only"):
        fz.differentiable(wave, t_pad=32)
    fz.win_length = 1024
    with pytest.raises(_native.SirError, match="HIP device"):     # the default front-end goes on to the argument checks
        fz.differentiable(wave, t_pad=32)
    assert featurizer.is_default_frontend(1024, 512) and not featurizer.is_default_frontend(1024, 256)
    # the library says the same (csrc/api.hip)
    src = open(os.path.join(ROOT, "speech-intent-recognizer_amd", "csrc", "api.hip")).read()
    assert "the waveform gradient is built for the default front-end only" in " ".join(src.replace('"', " ").split())


def test_header_declares_and_binding_carries_sir_create_ex():
    text = open(os.path.join(ROOT, "include", "sir_hip.h")).read()
    assert "the only size built" not in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+sir_create_ex\s*\(([^)]*)\)", text)
    assert m, "sir_create_ex is not declared in include/sir_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const sir_feature_config* cfg", "int win_length", "sir_handle** out"]
    res, argtypes = _native.SIGNATURES["sir_create_ex"]
    c_res, c_args = _native.SIGNATURES["sir_create"]
    assert res is c_res and len(argtypes) == 3 and argtypes[0] is c_args[0] and argtypes[2] is c_args[1]
    assert re.search(r"#define\s+SIR_ABI_VERSION\s+1\b", text)
    assert re.search(r"#define\s+SIR_PROFILE_EXTRA_IDS\s+1\b", text)


def test_predict_frontend_builds_one_extractor_per_front_end(monkeypatch):
    """scripts/predict_frontend.py (scripts/test_model.py keeps the reference's surface and front-end) hands its front-end to
    the extractor and pads to the caller's frame count; a failing file is None, never raised."""
    from sir_amd.scripts import predict_frontend as pf
    _bar_device(monkeypatch)
    made = _record_featurizers(monkeypatch)
    monkeypatch.setattr(pf, "_extractors", {})
    ex = pf.get_extractor({"n_fft": 512, "hop_length": 160, "win_length": 400})
    assert ex is pf.get_extractor(FrontEnd(512, 160, 400)) and ex is not pf.get_extractor(None)
    ex._featurizer()
    pf.get_extractor()._featurizer()
    assert made == [(16000, 64, 512, 160, 400), (16000, 64, 1024, 512, 1024)]
    seen = []

    class Ex:
        def extract_batch(self, paths, max_duration):
            return [torch.ones(64, 301), None]
    monkeypatch.setattr(pf, "get_extractor", lambda fe=None: seen.append(as_frontend(fe)) or Ex())
    monkeypatch.setattr(pf.ops, "check_status", lambda: None)

    def model(batch):
        seen.append(tuple(batch.shape))
        return torch.tensor([[0.0, 2.0, 1.0]])
    res = pf.predict_many(model, ["a.wav", "b.wav"], {"x": 0, "y": 1, "z": 2}, "cpu", pad_to=304, frontend=(512, 160, 400))
    assert seen == [FrontEnd(512, 160, 400), (1, 64, 304)]
    assert res[1] is None and res[0]["predicted_label"] == "y"
    assert pf.predict(model, "a.wav", {"x": 0, "y": 1, "z": 2}, "cpu", pad_to=304, frontend=(512, 160, 400))["predicted_label"] == "y"


def test_recogniser_pads_to_the_length_it_was_given():
    """``recognize_recordings`` / ``score_segments`` pad to the recogniser's own ``mel_spec_length`` unless told otherwise."""
    import inspect
    from sir_amd.scripts import testing
    for fn in (testing.IntentRecognizer.score_segments, testing.IntentRecognizer.recognize_recordings):
        assert inspect.signature(fn).parameters["pad_to"].default == testing.TRAINED_LENGTH
    reco = object.__new__(testing.IntentRecognizer)
    reco.label_map = {"a": 0}
    reco._finish(None, {"n_fft": 512, "hop_length": 160, "win_length": 400}, 304)
    assert reco.frontend == (512, 160, 400) and reco.mel_spec_length == 304
    assert reco.frontend.max_samples(reco.mel_spec_length) == 304 * 160 - 1
    reco._finish(None)
    assert reco.frontend.is_default and reco.mel_spec_length == testing.MAX_LENGTH == 200
