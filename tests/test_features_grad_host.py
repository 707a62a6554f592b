"""CPU: the reference of the waveform gradient is sound, and the surface exists and refuses bad arguments before any device
call -- ``tests/features_grad_ref.py`` against the numpy oracle and ``gradcheck``, the header and the binding table,
``HipFeaturizer.differentiable`` and ``sir_amd.explain.wave_gradient`` / ``fgsm_wave`` with every device call barred."""
import os
import re

import numpy as np
import pytest
import torch

import features_grad_ref as ref
from oracle import features_ref
from sir_amd import _native
from sir_amd.models.models import CNNAudioGRU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [513, 1500, 8192])
def test_restatement_agrees_with_the_numpy_oracle(n):
    x = ref.tones_and_noise(n, seed=n).double()
    got = ref.features_f64(x).numpy()
    want = features_ref.extract_features_f64(x.numpy())
    assert got.shape == want.shape == (64, 1 + n // 512)
    assert np.abs(got - want).max() <= 1e-9


def test_restatement_pads_masks_and_shifts():
    x = ref.tones_and_noise(3000, seed=5).double()
    out = ref.features_f64(x, t_pad=12, time_mask=(2, 3), freq_mask=(10, 6))
    plain = ref.features_f64(x)
    assert out.shape == (64, 12) and (out[:, 6:] == 0).all() and (out[:, 2:5] == 0).all() and (out[10:16] == 0).all()
    assert torch.equal(out[:10, :2], plain[:10, :2]) and torch.equal(out[16:, 5], plain[16:, 5])
    s = ref.shifted(x, 300)
    assert (s[:300] == 0).all() and torch.equal(s[300:], x[:-300])
    s = ref.shifted(x, -700)
    assert (s[-700:] == 0).all() and torch.equal(s[:-700], x[700:])
    assert torch.equal(ref.features_f64(x, shift=300), ref.features_f64(ref.shifted(x, 300)))


def test_reference_gradient_passes_gradcheck():
    x = ref.tones_and_noise(1500, seed=7).double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda w: ref.features_f64(w, t_pad=8, time_mask=(1, 1), freq_mask=(3, 2)), (x,),
                                    eps=1e-6, atol=1e-5, rtol=1e-4, fast_mode=True)


def test_constant_tile_rule_and_float32_yardstick():
    """All-zero clip: every mel value is under the clamp, the dB tile is constant, and the stated rule gives a zero, finite
    gradient.  The float32 yardstick differentiates the same function (it lands within float32 reach of the float64 one)."""
    dout = torch.randn(64, 8, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    g = ref.grad_f64(torch.zeros(2048), dout)
    assert g.shape == (2048,) and (g == 0).all()
    x = ref.tones_and_noise(1500, seed=9)
    g64, g32 = ref.grad_f64(x, dout), ref.grad_f32(x, dout)
    assert 0.0 < ref.clip_error(g32, g64) < 1e-3


def test_header_declares_and_binding_carries_the_entry_point():
    text = open(os.path.join(ROOT, "include", "sir_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+sir_features_bwd\s*\(([^)]*)\)", text)
    assert m, "sir_features_bwd is not declared in include/sir_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 14
    assert args[7] == "const float* db" and args[8] == "const float* dout" and args[11] == "float* dwave" and args[13] == "void* stream"
    res, argtypes = _native.SIGNATURES["sir_features_bwd"]
    fwd_res, fwd_args = _native.SIGNATURES["sir_features_fwd"]
    assert res is fwd_res and len(argtypes) == 14 and argtypes[:7] == fwd_args[:7]
    assert re.search(r"#define\s+SIR_ABI_VERSION\s+1\b", text)
    assert re.search(r"#define\s+SIR_PROFILE_EXTRA_IDS\s+1\b", text)      # no profile id was added


@pytest.fixture(scope="module")
def model():
    return CNNAudioGRU(31)


def _bar_device(monkeypatch):
    from sir_amd import featurizer

    def no_device(*a, **k):
        raise AssertionError("a device call was made before the arguments were validated")

    monkeypatch.setattr(featurizer, "get_featurizer", no_device)
    monkeypatch.setattr(_native, "lib", no_device)


def test_explain_wave_functions_validate_before_any_device_call(model, monkeypatch):
    from sir_amd import explain
    _bar_device(monkeypatch)
    wave = torch.zeros(2, 4000)
    labels = torch.tensor([0, 1])
    for call in (lambda: explain.wave_gradient(model, wave, t_pad=16), lambda: explain.fgsm_wave(model, wave, labels, 1e-3, t_pad=16)):
        with pytest.raises(_native.SirError):                # CPU tensors
            call()
    for bad_eps in (-1e-3, float("nan")):
        with pytest.raises(ValueError):
            explain.fgsm_wave(model, wave, labels, bad_eps, t_pad=16)
    # the checks below come before the device check
    for bad in (wave.to(torch.int16), wave.double(), torch.zeros(4000), torch.zeros(2, 1, 4000)):
        with pytest.raises(ValueError):
            explain.wave_gradient(model, bad, t_pad=16)
        with pytest.raises(ValueError):
            explain.fgsm_wave(model, bad, labels, 1e-3, t_pad=16)
    with pytest.raises(ValueError):                          # 1 + 4000 // 512 = 8 frames
        explain.wave_gradient(model, wave, t_pad=7)
    with pytest.raises(ValueError):                          # 17 frames
        explain.fgsm_wave(model, torch.zeros(2, 8192), labels, 1e-3, t_pad=16)
    with pytest.raises(ValueError):
        explain.wave_gradient(model, wave, lengths=torch.tensor([4000]), t_pad=16)
    with pytest.raises(ValueError):
        explain.wave_gradient(model, wave, lengths=torch.tensor([4000.0, 4000.0]), t_pad=16)
    with pytest.raises(ValueError):
        explain.fgsm_wave(model, wave, labels, 1e-3, t_pad=16, clamp=(1.0, -1.0))


def test_wave_target_and_labels_are_checked(model, monkeypatch):
    from sir_amd import explain
    _bar_device(monkeypatch)
    monkeypatch.setattr(explain, "_on_device", lambda model, x: True)
    wave = torch.zeros(2, 4000)
    for bad in (torch.tensor([1, 2, 3]), torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]]), torch.tensor([0, 31]), [0, -1]):
        with pytest.raises(ValueError):
            explain.wave_gradient(model, wave, target=bad, t_pad=16)
    for bad in (torch.tensor([1]), torch.tensor([True, False]), torch.tensor([0, 31])):
        with pytest.raises(ValueError):
            explain.fgsm_wave(model, wave, bad, 1e-2, t_pad=16)


def test_differentiable_validates_before_any_device_call(monkeypatch):
    from sir_amd import featurizer
    _bar_device(monkeypatch)
    fz = object.__new__(featurizer.HipFeaturizer)            # (no handle: creating one is a device call)
    fz.hop_length, fz.n_mels, fz._h = 512, 64, None
    wave = torch.zeros(2, 4000)
    with pytest.raises(_native.SirError, match="HIP device"):
        fz.differentiable(wave, t_pad=16)                    # CPU tensor
    with pytest.raises(_native.SirError, match="int16"):
        fz.differentiable(wave.to(torch.int16), t_pad=16)    # an int16 leaf cannot carry a gradient
    with pytest.raises(_native.SirError, match="frames"):
        fz.differentiable(wave, t_pad=7)                     # clip too long for t_pad
    with pytest.raises(_native.SirError):
        fz.differentiable(torch.zeros(4000), t_pad=16)
    with pytest.raises(_native.SirError):
        fz.differentiable(wave, lengths=torch.tensor([4000]), t_pad=16)
