"""Fine-tuning a checkpoint on a new label set: keep the body, give it a fresh head, freeze what should stay fixed.

The workflow the reference is built around -- its FSC checkpoint adapted to a handful of custom intents with a few
hundred clips -- is the torch recipe

    model.load_state_dict(pretrained)          # then a fresh fc for the new label set
    model.train()
    for bn in (model.bn1, model.bn2, model.bn3): bn.eval()
    for p in cnn_params: p.requires_grad_(False)

``load_pretrained`` is its first line for a checkpoint whose ``num_classes`` differs, ``freeze`` the rest.  The training step
honours the flags per sub-module (``train_ops.forward_train``) and its backward stops where the trainable parameters stop.
Nothing here touches the GPU: both helpers work on CPU and meta tensors too.
"""
import math

import torch
from torch import nn

FREEZE_CHOICES = ("bn_stats", "cnn", "gru", "attention")
_BN = ("bn1", "bn2", "bn3")


def _unwrap(state):
    """A raw state dict or a training checkpoint ``{'model_state_dict': ...}`` (the reference's two loaders:
    scripts/evaluate.py reads the former, scripts/test_model.py the latter)."""
    if isinstance(state, (str, bytes)) or hasattr(state, "__fspath__"):
        state = torch.load(state, map_location="cpu", weights_only=True)
    if isinstance(state, dict) and "model_state_dict" in state:
        state = state["model_state_dict"]
    if not isinstance(state, dict):
        raise TypeError("expected a state dict, a {'model_state_dict': ...} checkpoint or a path to one")
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}


def reset_linear_(linear):
    """``nn.Linear.reset_parameters`` (torch's default init: kaiming_uniform(a=sqrt(5)) weight, uniform(+-1/sqrt(fan_in)) bias)."""
    with torch.no_grad():
        nn.init.kaiming_uniform_(linear.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(linear.weight.shape[1])
        nn.init.uniform_(linear.bias, -bound, bound)


def load_pretrained(model, state, reset_head=None):
    """Copy every tensor of ``state`` whose key and shape match ``model`` into it; leave the rest of ``model`` alone.

    ``reset_head``: ``None`` (default) re-initialises ``fc`` with torch's default init exactly when the checkpoint's
    ``fc`` does not fit (another ``num_classes``) or is missing; ``True`` always; ``False`` never (a mismatching ``fc`` is
    then simply left as constructed).  Returns a report: ``{"kept": [...], "reset": [...], "missing": [...],
    "unexpected": [...], "shape_mismatch": [...]}`` -- keys copied, keys re-initialised, model keys the checkpoint lacks,
    checkpoint keys the model lacks, keys present on both sides with different shapes."""
    src = _unwrap(state)
    own = model.state_dict()
    kept, mismatch = [], []
    missing = [k for k in own if k not in src]
    unexpected = [k for k in src if k not in own]
    head = ("fc.weight", "fc.bias")
    for k, t in own.items():
        if k not in src:
            continue
        if tuple(src[k].shape) != tuple(t.shape):
            mismatch.append(k)
        elif not (reset_head is True and k in head):
            kept.append(k)
    bad = [k for k in mismatch if k not in head]
    if bad:
        raise ValueError(f"checkpoint tensors do not fit the model (only fc may differ): {bad}")
    # (load_state_dict(strict=False) on the matching subset: the model's own hook drops its cached pointer struct)
    model.load_state_dict({k: src[k] for k in kept}, strict=False)
    reset = []
    head_fits = all(k in kept for k in head)
    if reset_head is True or (reset_head is None and not head_fits):
        reset_linear_(model.fc)
        kept = [k for k in kept if k not in head]
        reset = list(head)
    return {"kept": kept, "reset": reset, "missing": missing, "unexpected": unexpected, "shape_mismatch": mismatch}


def freeze(model, what):
    """Freeze parts of ``model`` for fine-tuning.  ``what`` is a subset of

    - ``"bn_stats"``: ``bn1..3.eval()`` -- the pretrained running statistics are used and kept; gamma / beta still train
      unless ``"cnn"`` is frozen too.  ``CNNAudioGRU.train()`` re-applies this, so the per-epoch ``model.train()`` does
      not undo it (on a plain ``nn.Module`` the torch idiom is to call ``bn.eval()`` again after every ``train()``).
    - ``"cnn"``: ``requires_grad_(False)`` on conv1..3.weight and bn1..3.weight / bias.
    - ``"gru"``: ``requires_grad_(False)`` on all 16 GRU tensors, and ``gru.eval()`` (no inter-layer dropout).
    - ``"attention"``: ``requires_grad_(False)`` on attention.weight / bias.

    ``fc`` always stays trainable.  Returns the names of the parameters that are still trainable."""
    what = set([what] if isinstance(what, str) else what)
    unknown = what - set(FREEZE_CHOICES)
    if unknown:
        raise ValueError(f"freeze: unknown {sorted(unknown)}; choose from {FREEZE_CHOICES}")
    frozen_modules = set(getattr(model, "_sir_frozen_modules", ()))
    if "bn_stats" in what:
        frozen_modules.update(_BN)
    if "gru" in what:
        frozen_modules.add("gru")
    model._sir_frozen_modules = tuple(sorted(frozen_modules))
    for name in model._sir_frozen_modules:
        getattr(model, name).eval()
    prefixes = ()
    if "cnn" in what:
        prefixes += ("conv", "bn")
    if "gru" in what:
        prefixes += ("gru.",)
    if "attention" in what:
        prefixes += ("attention.",)
    for n, p in model.named_parameters():
        if prefixes and n.startswith(prefixes):
            p.requires_grad_(False)
    return [n for n, p in model.named_parameters() if p.requires_grad]


def trainable_parameters(model):
    """The parameters an optimizer should be built over after ``freeze``."""
    return [p for p in model.parameters() if p.requires_grad]
