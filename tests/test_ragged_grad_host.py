"""Host side of the ragged differentiable path (no GPU): the two new C symbols, the three new ``sir_amd.explain`` functions and
their validation (before any device call), the refusal of ``lengths=`` with live batch statistics, and the float64 statement the
kernels implement -- the masked dense form equals the per-clip reference (tests/ragged_grad_ref.py)."""
import ctypes
import inspect
import os

import pytest
import torch

import ragged_grad_ref as rg
from oracle import model_ref
from sir_amd import _native, explain, synth
from sir_amd.models.models import CNNAudioGRU


def test_library_exports_the_ragged_step():
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in ("sir_model_train_fwd_ragged", "sir_model_train_bwd_ragged"):
        assert hasattr(handle, name), name
        assert name in _native.SIGNATURES
    assert _native.lib().sir_abi_version() == 1
    # the profile id space did not grow: new launches run inside existing scopes or carry no id
    assert _native.PROFILE_EXTRA_IDS == 1


def test_explain_ragged_functions_exist():
    assert list(inspect.signature(explain.input_gradient_ragged).parameters) == ["model", "x", "frames", "target"]
    assert list(inspect.signature(explain.saliency_ragged).parameters) == ["model", "x", "frames", "target"]
    assert list(inspect.signature(explain.fgsm_ragged).parameters) == ["model", "x", "labels", "eps", "frames"]
    from sir_amd import train_ops
    assert list(inspect.signature(train_ops.forward_train).parameters) == ["mod", "x", "lengths"]


@pytest.fixture()
def no_device(monkeypatch):
    """Any device call from here on is a test failure: the library and the featurizer are barred."""
    def barred(*a, **k):
        raise AssertionError("a device call was made before the arguments were validated")
    from sir_amd import featurizer
    monkeypatch.setattr(_native, "lib", barred)
    monkeypatch.setattr(featurizer, "get_featurizer", barred)


def _calls(m, x, frames):
    return [lambda: explain.input_gradient_ragged(m, x, frames), lambda: explain.saliency_ragged(m, x, frames),
            lambda: explain.fgsm_ragged(m, x, [0] * x.shape[0], 0.1, frames)]


def test_explain_ragged_validates_before_any_device_call(no_device):
    m = CNNAudioGRU(31)
    x = torch.zeros(3, 64, 24)
    for bad in ([24, 8], [24, 8, 16, 9], torch.tensor([[24, 8, 16]]), None):               # wrong length / shape / missing
        for call in _calls(m, x, bad):
            with pytest.raises(ValueError, match="frames"):
                call()
    for bad in ([24.0, 8.0, 16.0], torch.tensor([24.0, 8.0, 16.0]), torch.tensor([True, True, False])):   # wrong dtype
        for call in _calls(m, x, bad):
            with pytest.raises(ValueError, match="integers"):
                call()
    for bad in ([24, 7, 16], [25, 8, 16], torch.tensor([24, 8, -1])):                        # a host value outside [8, T]
        for call in _calls(m, x, bad):
            with pytest.raises(ValueError, match=r"outside \[8, 24\]"):
                call()
    for call in _calls(m, torch.zeros(3, 64, 24, dtype=torch.float64), [24, 8, 16]):
        with pytest.raises(ValueError, match="float32"):
            call()
    for call in _calls(m, torch.zeros(3, 32, 24), [24, 8, 16]):
        with pytest.raises(ValueError, match="expected"):
            call()
    with pytest.raises(ValueError, match="target"):
        explain.input_gradient_ragged(m, x, [24, 8, 16], target=[0, 1, 31])
    with pytest.raises(ValueError, match="labels"):
        explain.fgsm_ragged(m, x, [0, 1], 0.1, [24, 8, 16])
    with pytest.raises(ValueError, match="eps"):
        explain.fgsm_ragged(m, x, [0, 1, 2], -1.0, [24, 8, 16])
    for call in _calls(m, x, [24, 8, 16]):                                                   # valid arguments, CPU tensors
        with pytest.raises(_native.SirError, match="HIP device"):
            call()


def test_padded_forms_keep_refusing_lengths(no_device):
    m = CNNAudioGRU(31)
    x = torch.zeros(2, 64, 16)
    for call in (lambda: explain.input_gradient(m, x, lengths=[16, 8]), lambda: explain.saliency(m, x, lengths=[16, 8]),
                 lambda: explain.fgsm(m, x, [0, 1], 0.1, lengths=[16, 8]), lambda: explain.pgd(m, x, [0, 1], 0.1, lengths=[16, 8])):
        with pytest.raises(ValueError, match="lengths"):
            call()


def test_lengths_with_live_statistics_raise(no_device):
    m = CNNAudioGRU(31).train()
    x = torch.zeros(2, 64, 16)
    with torch.enable_grad():
        for lengths in ([16, 8], torch.tensor([16, 8])):
            with pytest.raises(_native.SirError, match="lengths") as e:
                m(x, lengths=lengths)
            assert "freeze" in str(e.value)
        m.bn1.eval(); m.bn2.eval()                       # one live block is enough
        with pytest.raises(_native.SirError, match="lengths"):
            m(x, lengths=[16, 8])


def test_masked_dense_form_equals_the_per_clip_reference():
    """float64, batch 10, t_frames 40, dropout 0.5: the masked dense statement (ragged_grad_ref.masked_dense, this suite's own code)
    against per-clip ``oracle.model_ref.forward(..., train=False)`` under autograd.  Measured: logits 2e-15, dx and every parameter
    gradient below 6e-14 of their rms.  Bounds: 1e-12 / 1e-11 -- float64's 2.2e-16 times the ~1e4 terms of the longest sums, with
    room for their different orders; nothing derived from a device."""
    sd = synth.synth_state_dict(31, seed=0)
    frames = rg.CASE_FRAMES
    g = torch.Generator().manual_seed(5)
    x = torch.randn(10, 64, 40, generator=g)
    labels = torch.randint(0, 31, (10,), generator=g)
    mask = (torch.rand(10, 5, 512, generator=g) >= 0.5).double() * 2.0
    ref_loss, ref_logits, ref_grads, ref_dx = rg.per_clip_reference(sd, x, frames, labels, dropout_mask=mask)
    xn = x.clone()
    for b, f in enumerate(frames):
        xn[b, :, f:] = float("nan")                      # the masked form selects, it does not multiply
    loss, logits, grads, dx = rg.masked_dense(sd, xn, frames, labels, dropout_mask=mask)
    lg = (logits - ref_logits).abs().max().item()
    r = rg.grad_ratios(grads, ref_grads)
    r["dx"] = rg.ratio(dx, ref_dx)
    print(f"masked dense vs per clip: logits {lg:.1e}, worst gradient {max(r.values()):.1e}", {k: f"{v:.0e}" for k, v in r.items()})
    assert "attention.bias" not in r and len(r) == 29
    assert lg <= 1e-12 and abs(loss.item() - ref_loss.item()) <= 1e-12
    assert max(r.values()) <= 1e-11, r
    for b, f in enumerate(frames):
        assert torch.equal(dx[b, :, f:], torch.zeros_like(dx[b, :, f:]))
        if f % 2:                                        # the pool drops an odd last column, conv1 still reads it
            assert dx[b, :, f - 1].abs().max() > 0
