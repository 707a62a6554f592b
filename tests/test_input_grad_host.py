"""CPU: the input-gradient surface exists and refuses bad arguments before any device call -- ``sir_amd.explain`` imports
without a GPU, the header declares ``sir_model_train_bwd_x`` and the binding table carries it."""
import os
import re

import pytest
import torch

from sir_amd import _native
from sir_amd.models.models import CNNAudioGRU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_binding_carries_the_entry_point():
    text = open(os.path.join(ROOT, "include", "sir_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+sir_model_train_bwd_x\s*\(([^)]*)\)", text)
    assert m, "sir_model_train_bwd_x is not declared in include/sir_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 15 and args[10] == "float* dfeats"
    res, argtypes = _native.SIGNATURES["sir_model_train_bwd_x"]
    cfg_res, cfg_args = _native.SIGNATURES["sir_model_train_bwd_cfg"]
    assert res is cfg_res and len(argtypes) == 15
    assert argtypes[:10] == cfg_args[:10] and argtypes[11:] == cfg_args[10:]      # the _cfg call with dfeats put in
    assert re.search(r"#define\s+SIR_ABI_VERSION\s+1\b", text) or _native.lib().sir_abi_version() == 1


def test_profile_id_is_appended():
    """The new id is appended behind every existing one -- behind ``sir_profile_kernel_count()`` itself, which keeps its value, so
    that walks over ``range(count)`` (the benchmark's tables) see the list they always saw."""
    lib = _native.lib()
    n = lib.sir_profile_kernel_count()
    names = [lib.sir_profile_kernel_name(i).decode() for i in range(n + _native.PROFILE_EXTRA_IDS + 1)]
    assert n == 49 and _native.PROFILE_EXTRA_IDS == 1
    assert names[n] == "bwd_conv1_dgrad" and names.count("bwd_conv1_dgrad") == 1 and names[n + 1] == ""
    assert names[38] == "bwd_conv1" and names[n - 1] == "vad_gather"              # the earlier ids keep their numbers
    header = open(os.path.join(ROOT, "include", "sir_hip.h")).read()
    assert re.search(r"#define\s+SIR_PROFILE_EXTRA_IDS\s+1\b", header)


@pytest.fixture(scope="module")
def model():
    return CNNAudioGRU(31)


def test_explain_validates_before_any_device_call(model, monkeypatch):
    from sir_amd import explain, featurizer

    def no_device(*a, **k):
        raise AssertionError("a device call was made before the arguments were validated")

    monkeypatch.setattr(featurizer, "get_featurizer", no_device)
    monkeypatch.setattr(_native, "lib", no_device)
    x = torch.zeros(2, 64, 16)
    labels = torch.tensor([0, 1])
    for call in (lambda: explain.input_gradient(model, x), lambda: explain.saliency(model, x),
                 lambda: explain.fgsm(model, x, labels, 1e-2)):
        with pytest.raises(_native.SirError):                # CPU tensors
            call()
    with pytest.raises(ValueError):
        explain.fgsm(model, x, labels, -1e-3)
    with pytest.raises(ValueError):
        explain.fgsm(model, x, labels, float("nan"))
    for fn in (explain.input_gradient, explain.saliency):
        with pytest.raises(ValueError):
            fn(model, x, lengths=[16, 16])
    with pytest.raises(ValueError):
        explain.fgsm(model, x, labels, 1e-2, lengths=torch.tensor([16, 16]))
    # (the checks below come before the device check, so they can be exercised here; meta tensors stand in for nothing)
    with pytest.raises(ValueError):
        explain.input_gradient(model, torch.zeros(2, 3, 64, 16))
    with pytest.raises(ValueError):
        explain.input_gradient(model, torch.zeros(2, 64, 4))


def test_target_and_labels_are_checked(model, monkeypatch):
    """A ``target`` of the wrong length, of a float type or outside the classes raises ``ValueError`` (with tensors that pass
    the device check: the module and ``x`` are made to look resident, and every device call is barred)."""
    from sir_amd import explain, featurizer

    def no_device(*a, **k):
        raise AssertionError("a device call was made before the arguments were validated")

    monkeypatch.setattr(featurizer, "get_featurizer", no_device)
    monkeypatch.setattr(_native, "lib", no_device)
    monkeypatch.setattr(explain, "_on_device", lambda model, x: True)
    x = torch.zeros(2, 64, 16)
    for bad in (torch.tensor([1, 2, 3]), torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]]), torch.tensor([0, 31]), [0, -1]):
        with pytest.raises(ValueError):
            explain.input_gradient(model, x, bad)
    for bad in (torch.tensor([1]), torch.tensor([True, False])):
        with pytest.raises(ValueError):
            explain.fgsm(model, x, bad, 1e-2)
