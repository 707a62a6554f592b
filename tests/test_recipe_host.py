"""CPU: the float64 statement of the training recipe (tests/recipe_ref.py) against torch's own functions, the host side
of ``Mixup`` and the routing of a label-smoothed criterion.  No GPU is touched."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import recipe_ref
from sir_amd import train_ops
from sir_amd.scripts import train as tr


def _case(bsz, ncls, second, ignored, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(bsz, ncls, generator=g, dtype=torch.float64) * 3.0
    ya = torch.randint(0, ncls, (bsz,), generator=g)
    yb = torch.randint(0, ncls, (bsz,), generator=g) if second else None
    lam = torch.rand(bsz, generator=g, dtype=torch.float64) if second else None
    if second:
        lam[0], lam[1] = 0.0, 1.0
    if ignored:
        ya[2] = -100
        ya[bsz - 1] = -100
    return logits, ya, yb, lam


def _torch_two_term(logits, ya, yb, lam, eps):
    """lam * F.cross_entropy(l, ya, label_smoothing=eps) + (1 - lam) * F.cross_entropy(l, yb, label_smoothing=eps) with a
    per-row lam: per-row losses weighed, mean over the rows ya does not ignore."""
    valid = ya != -100
    la = F.cross_entropy(logits, ya, reduction="none", label_smoothing=eps)
    if yb is None:
        return la.sum() / valid.sum()
    lb = F.cross_entropy(logits, torch.where(valid, yb, torch.zeros_like(yb)), reduction="none", label_smoothing=eps)
    return ((lam * la + (1.0 - lam) * lb) * valid).sum() / valid.sum()


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("ignored", [False, True])
def test_soft_ce_equals_torch_two_term_form(eps, second, ignored):
    for bsz, ncls in ((5, 6), (8, 31)):
        logits, ya, yb, lam = _case(bsz, ncls, second, ignored, seed=bsz)
        lg = logits.clone().requires_grad_(True)
        ref = _torch_two_term(lg, ya, yb, lam, eps)
        ref.backward()
        loss, dlogits = recipe_ref.soft_ce(logits, ya, yb, lam, eps)
        assert abs(loss.item() - ref.item()) <= 1e-12
        assert (dlogits - lg.grad).abs().max().item() <= 1e-12


@pytest.mark.parametrize("factor", [0.5, 1.0, 2.0])            # total norm below, at and above max_norm
def test_clip_equals_clip_grad_norm(factor):
    g = torch.Generator().manual_seed(3)
    grads = [torch.randn(n, generator=g, dtype=torch.float64) for n in (1, 5, 4097, 300)]
    norm = torch.sqrt(sum((x ** 2).sum() for x in grads)).item()
    max_norm = norm / factor
    params = [nn.Parameter(torch.zeros_like(x)) for x in grads]
    for p, x in zip(params, grads):
        p.grad = x.clone()
    ref_norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
    total, coef, scaled = recipe_ref.clip(grads, max_norm)
    assert abs(total.item() - ref_norm.item()) <= 1e-12 * norm
    assert (coef.item() < 1.0) == (factor >= 1.0)             # at max_norm the + 1e-6 already makes coef < 1, as in torch
    for p, s in zip(params, scaled):
        assert (p.grad - s).abs().max().item() <= 1e-12


def test_mix_reference_is_the_convex_combination():
    x = torch.arange(24, dtype=torch.float32).view(4, 2, 3)
    perm = torch.tensor([1, 0, 3, 2])
    lam = torch.tensor([1.0, 0.0, 0.25, 0.5])
    out = recipe_ref.mix(x, perm, lam)
    assert torch.equal(out[0], x[0].double()) and torch.equal(out[1], x[0].double())
    assert torch.equal(out[2], 0.25 * x[2].double() + 0.75 * x[3].double())


def test_mixup_draws_on_the_host(monkeypatch):
    def no_cuda(*a, **k):
        raise AssertionError("Mixup.draw touched the device")
    monkeypatch.setattr(torch.cuda, "_lazy_init", no_cuda)
    a, b = train_ops.Mixup(0.2, seed=7), train_ops.Mixup(0.2, seed=7)
    other = train_ops.Mixup(0.2, seed=8)
    seq_a, seq_b, seq_o = [], [], []
    for bsz in (1, 5, 8, 256):
        for mx, seq in ((a, seq_a), (b, seq_b), (other, seq_o)):
            perm, lam = mx.draw(bsz)
            assert perm.dtype == torch.int64 and lam.dtype == torch.float32 and not perm.is_cuda and not lam.is_cuda
            assert sorted(perm.tolist()) == list(range(bsz))
            assert lam.shape == (bsz,) and (lam == lam[0]).all() and 0.0 <= float(lam[0]) <= 1.0
            seq.append((perm.tolist(), float(lam[0])))
    assert seq_a == seq_b and seq_a != seq_o
    with pytest.raises(ValueError):
        train_ops.Mixup(0.0)


def test_loss_fn_routes_label_smoothing_to_the_hip_loss():
    assert tr._loss_fn(nn.CrossEntropyLoss()) is train_ops.fused_cross_entropy
    fn = tr._loss_fn(nn.CrossEntropyLoss(label_smoothing=0.1))
    assert fn.func is train_ops.fused_cross_entropy and fn.keywords == {"label_smoothing": pytest.approx(0.1)}
    for crit in (nn.CrossEntropyLoss(weight=torch.ones(31)), nn.CrossEntropyLoss(reduction="sum"),
                 nn.CrossEntropyLoss(label_smoothing=0.1, reduction="none"), nn.CrossEntropyLoss(ignore_index=3),
                 nn.NLLLoss()):
        assert tr._loss_fn(crit) is crit


def test_epoch_signatures_keep_the_reference_order():
    import inspect
    assert list(inspect.signature(tr.train_epoch).parameters) == ["model", "train_loader", "optimizer", "criterion", "device",
                                                                  "scaler", "mixup"]
    assert list(inspect.signature(tr.train_epoch_waveforms).parameters)[-1] == "mixup"
    from sir_amd.optim import FusedAdam
    with pytest.raises(ValueError):
        FusedAdam([nn.Parameter(torch.zeros(3))], max_grad_norm=0.0)
    assert FusedAdam([nn.Parameter(torch.zeros(3))]).max_grad_norm is None
