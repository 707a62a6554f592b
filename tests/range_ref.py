"""Shared pieces of the operand-range tests (``test_operand_range_gpu.py``).

The one thing added to the suite's oracle: ``TrainOracle`` differentiates ``oracle.model_ref.forward`` for an ARBITRARY upstream
gradient, ``(logits * dlogits).sum()``, instead of the mean cross-entropy -- on the device the same is ``logits.backward(dlogits)``.
As everywhere in this suite it is evaluated in float64 at the device's own ReLU / max-pool values (``z_override`` /
``y_override``, ``train_step_ref._device_forward_values``).  The forward graph is built once and kept, so one forward serves
several upstream gradients; the oracle is linear in ``dlogits``, which lets a test scale one reference by an exact power of two.

``backward_errors`` is the comparison of ``train_step_ref._training_case`` for such a backward: the 29 parameter gradients
through ``_grad_errors`` (max |a - b| / rms, absolute where the reference is zero), their norms, and the five stage gradients of
the workspace divided by the loss scale the device used (slot 39, ``device_loss_scale``).
"""
import ctypes as C
import types

import torch

from oracle import model_ref
from sir_amd import _native
from sir_amd.featurizer import get_featurizer
from train_step_ref import _grad_errors, _rel

GRAD_BOUND = 2e-3          # max |a - b| <= GRAD_BOUND * rms(reference): the project's gradient bound (_training_case)
NORM_BOUND = 1e-3          # | |a| - |b| | <= NORM_BOUND * |b| + 1e-7
STAGES = {"dy1": "gru_l1", "dy0": "gru_l0", "dx0": "gru_in", "da2": "conv2", "da1": "conv1"}      # workspace slot -> oracle stage


class TrainOracle:
    """``model_ref.forward`` in ``dtype`` at the device's forward values, differentiable for any ``dlogits``.  ``train``: batch
    statistics (True) or the running ones (False) in all three BatchNorms."""

    def __init__(self, sd, x, zo, yo, dtype=torch.float64, train=True):
        c = lambda v: v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v
        self.dtype = dtype
        self.params = {k: c(sd[k]).detach().clone().requires_grad_(True) for k in model_ref.PARAM_KEYS}
        full = {k: c(v) for k, v in sd.items()}
        full.update(self.params)
        self.stages = {}
        self.logits = model_ref.forward(full, c(x), train=train, stages=self.stages, z_override={k: c(v) for k, v in zo.items()},
                                        y_override={k: c(v) for k, v in yo.items()})

    def vjp(self, dlogits):
        """``(grads {parameter: tensor}, stage gradients {slot name: tensor, NHWC for the conv stages})`` of
        ``(logits * dlogits).sum()``."""
        out = (self.logits * dlogits.detach().cpu().to(self.dtype)).sum()
        names = list(STAGES)
        got = torch.autograd.grad(out, [self.params[k] for k in model_ref.PARAM_KEYS] + [self.stages[STAGES[n]] for n in names],
                                  retain_graph=True)
        grads = dict(zip(model_ref.PARAM_KEYS, got))
        st = dict(zip(names, got[len(model_ref.PARAM_KEYS):]))
        for n in ("da2", "da1"):
            st[n] = st[n].permute(0, 2, 3, 1)
        return grads, st


def device_loss_scale(m, bsz, t, row=None):
    """The loss scale the device's last backward of ``m`` used (workspace slot 39: pair 0, or pair ``1 + row``)."""
    offs = (C.c_size_t * 48)()
    n = _native.lib().sir_model_train_workspace_offsets(get_featurizer().handle, bsz, t, offs, 48)
    assert n > 39
    pairs = m._sir_train["ws"].buf[offs[39]: offs[39] + 8 * (1 + bsz)].view(torch.float32).cpu()
    i = 0 if row is None else 1 + row
    scale, inv = pairs[2 * i].item(), pairs[2 * i + 1].item()
    assert scale * inv == 1.0
    return scale


def _scaled(m, factor):
    """``m`` as ``_grad_errors`` reads it, every gradient multiplied by ``factor`` in float64 (a power of two: exact)."""
    ps = [(n, types.SimpleNamespace(grad=p.grad.detach().cpu().double() * factor)) for n, p in m.named_parameters()]
    return types.SimpleNamespace(named_parameters=lambda: iter(ps))


def backward_errors(m, ref_grads, factor=1.0, views=None, ref_stages=None, stage_scale=None):
    """Per-tensor figures of the device's gradients times ``factor`` against ``ref_grads``: ``(gerr, nerr, serr)`` -- max |a - b| /
    rms (``_grad_errors``), relative norm error (tensors that are zero in exact arithmetic left out, as in ``_training_case``)
    and, with ``views``, the stage gradients divided by ``stage_scale``."""
    sm = _scaled(m, factor)
    gerr = _grad_errors(sm, ref_grads)
    nerr = {}
    for n, p in sm.named_parameters():
        rn = ref_grads[n].double().norm().item()
        nerr[n] = (abs(p.grad.norm().item() - rn), rn)
    serr = {}
    if views is not None:
        serr = {k: _rel(views[k].double() / stage_scale, r)[0] for k, r in ref_stages.items()}
    return gerr, nerr, serr


def assert_backward(tag, gerr, nerr, serr, bound=None, norm_bound=None, norm_atol=None):
    """Prints the figures, then holds them to ``GRAD_BOUND`` / ``NORM_BOUND`` (or the per-tensor ``bound`` / ``norm_bound``).
    ``norm_atol`` {name: absolute term in place of 1e-7} is ``_training_case``'s: for a gradient that is zero in exact arithmetic,
    where the float32 oracle's own rounding noise exceeds 1e-7 (the caller prints both)."""
    worst = max(gerr, key=gerr.get)
    rel_n = {n: d / rn for n, (d, rn) in nerr.items() if rn > 1e-7}
    print(f"{tag}: worst gradient {gerr[worst]:.1e} * rms ({worst}), worst norm {max(rel_n.values()):.1e}"
          + (", stage gradients / scale: " + str({k: f"{e:.1e}" for k, e in serr.items()}) if serr else ""))
    assert len(gerr) == 29
    for k, e in gerr.items():
        assert e == e and e < (bound or {}).get(k, GRAD_BOUND), (tag, k, e)
    for n, (d, rn) in nerr.items():
        assert d <= (norm_bound or {}).get(n, NORM_BOUND) * rn + (norm_atol or {}).get(n, 1e-7), (tag, n, d, rn)
    for k, e in serr.items():
        assert e == e and e < GRAD_BOUND, (tag, k, e)
    return gerr[worst]
