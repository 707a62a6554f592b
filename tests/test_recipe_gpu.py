"""GPU: the training recipe -- soft-target cross-entropy (label smoothing, mixup's two labels), batch mixing, global
gradient-norm clipping and the clipped Adam step -- against the float64 statement in tests/recipe_ref.py (itself checked
against torch's own functions in tests/test_recipe_host.py), and through the entry points."""
import ctypes as C
import json
import os
import types

import numpy as np
import pandas as pd
import pytest
import torch
import torch.nn.functional as F

import cases
import recipe_ref
from oracle import model_ref
from sir_amd import _native, ops, synth, train_ops
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU
from sir_amd.optim import FusedAdam

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                     # unit roundoff of fp32 (round to nearest)


@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(31, seed=0)


def _model(sd, dropout=0.0):
    m = CNNAudioGRU(31)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.gru.dropout = dropout
    return m


# ---- 1. loss ---------------------------------------------------------------------------------------------------------
_loss_case = recipe_ref.loss_case


def _dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("bsz", [5, 8, 256])
@pytest.mark.parametrize("ncls", [6, 31])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("second", [False, True])
def test_soft_loss_and_gradient_vs_float64(bsz, ncls, eps, second):
    """Loss within 1e-5 absolute (the bound of every existing loss comparison).  dlogits per element within
    (C + 8 + R) * 2^-24 / n_valid, R = max - min of the row's logits.  The kernel's operation count, in units of 2^-24 on a
    value <= 1: the exp argument l - max is rounded once (<= R/2 after the exponential), expf (<= 2), the C-term sum of
    the denominator (<= C/2), reciprocal and product (1), the target q from eps / C, (1 - eps) lam and (1 - eps)(1 - lam)
    and two additions (<= 2.5), the subtraction (0.5), grad_scale / n_valid and the final product (1):
    C/2 + R/2 + 7 <= C + 8 + R."""
    logits, ya, yb, lam = _loss_case(bsz, ncls, second, seed=17 * bsz + ncls)
    lg = logits.to(DEV).requires_grad_(True)
    loss = train_ops.fused_cross_entropy(lg, _dev(ya), _dev(yb), _dev(lam), label_smoothing=eps)
    loss.backward()
    ref_loss, ref_d = recipe_ref.soft_ce(logits, ya, yb, lam, eps)
    n_valid = int((ya != -100).sum())
    err = abs(loss.item() - ref_loss.item())
    spread = (logits.max(dim=1).values - logits.min(dim=1).values).double()[:, None]
    bound = (ncls + 8 + spread) * U / n_valid
    derr = (lg.grad.cpu().double() - ref_d).abs()
    print(f"soft CE B={bsz} C={ncls} eps={eps} second={second}: |loss - ref| {err:.3e}, "
          f"max dlogits err / bound {(derr / bound).max().item():.3f}")
    assert err <= 1e-5
    assert (derr <= bound).all()
    assert (lg.grad[ya.to(DEV) == -100] == 0).all()
    ops.check_status()


@pytest.mark.parametrize("bsz,ncls", [(5, 6), (8, 31), (256, 31), (16, 40)])
def test_hard_target_through_the_soft_entry_is_bit_identical_to_ce_loss(bsz, ncls):
    lib, h = _native.lib(), get_featurizer().handle
    logits, ya, _, _ = _loss_case(bsz, ncls, False, seed=5)
    lg, y = logits.to(DEV), ya.to(DEV)
    out = []
    for soft in (False, True):
        loss = torch.full((1,), -1.0, device=DEV)
        d = torch.full_like(lg, -1.0)
        if soft:
            rc = lib.sir_ce_loss_soft(h, lg.data_ptr(), y.data_ptr(), None, None, 0.0, bsz, ncls, loss.data_ptr(), d.data_ptr(),
                                      3.0, _native.current_stream_ptr())
        else:
            rc = lib.sir_ce_loss(h, lg.data_ptr(), y.data_ptr(), bsz, ncls, loss.data_ptr(), d.data_ptr(), 3.0,
                                 _native.current_stream_ptr())
        _native.check(rc, "ce")
        out.append((loss, d))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    # ... and the Python wrapper's two-argument call is that same launch
    assert torch.equal(train_ops.fused_cross_entropy(lg, y), train_ops.fused_cross_entropy(lg, y, None, None, 0.0))
    ops.check_status()


def test_bad_second_label_is_flagged():
    logits, ya, yb, lam = _loss_case(8, 31, True, seed=1)
    yb[4] = 31
    loss = train_ops.fused_cross_entropy(logits.to(DEV), ya.to(DEV), yb.to(DEV), lam.to(DEV), label_smoothing=0.1)
    assert torch.isnan(loss).item()
    with pytest.raises(_native.SirError):
        ops.check_status()
    with pytest.raises(_native.SirError):
        train_ops.fused_cross_entropy(logits.to(DEV), ya.to(DEV), label_smoothing=1.0)
    ops.check_status()


# ---- 2. mix ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(256, 64, 200), (5, 64, 96)])
def test_mix_features_vs_float64(shape):
    """|out - ref64| <= 2 * 2^-24 * (|lam a| + |(1 - lam) b|): the arithmetic is fixed as fmaf(lam, a, (1.0f - lam) * b), the
    product is rounded once and the fma once.  That count takes the complement as the kernel forms it, the fp32
    difference 1.0f - lam (exact for lam >= 0.5, Sterbenz), so the first assertion uses that value in the float64
    reference.  Against the real-number 1 - lam the complement's own rounding, delta_b = fl(1 - lam_b) - (1 - lam_b),
    known exactly per row and <= 2^-24 relative, adds |delta_b| |b| and nothing else: the second assertion."""
    bsz = shape[0]
    g = torch.Generator().manual_seed(bsz)
    x = torch.randn(shape, generator=g) * 4.0
    perm = torch.randperm(bsz, generator=g)
    lam = torch.rand(bsz, generator=g)
    lam[0], lam[1], lam[2] = 1.0, 0.0, 0.5
    out = train_ops.mix_features(x.to(DEV), perm.to(DEV), lam.to(DEV)).cpu()
    om32 = 1.0 - lam                                                  # fp32, one rounding
    l, om = lam.double().view(-1, 1, 1), om32.double().view(-1, 1, 1)
    a, b = x.double(), x.double()[perm]
    bound = 2 * U * ((l * a).abs() + (om * b).abs())
    err = (out.double() - recipe_ref.mix(x, perm, lam, complement=om32)).abs()
    delta = (om - (1.0 - l)).abs()
    assert (delta <= U * (1.0 - l)).all()
    err_def = (out.double() - recipe_ref.mix(x, perm, lam)).abs()
    bound_def = 2 * U * ((l * a).abs() + ((1.0 - l) * b).abs()) + delta * b.abs()
    print(f"mix {shape}: max err / bound {(err / bound.clamp(min=1e-300)).max().item():.3f}, against the real-number "
          f"complement {(err_def / bound_def.clamp(min=1e-300)).max().item():.3f}")
    assert (err <= bound).all()
    assert (err_def <= bound_def).all()
    assert torch.equal(out[0], x[0])
    ident = train_ops.mix_features(x.to(DEV), torch.arange(bsz, device=DEV), lam.to(DEV)).cpu()
    # identity permutation: the same two roundings around a * (lam + (1.0f - lam)), whose distance from a is known exactly
    assert ((ident.double() - a).abs() <= (2 * U * (l.abs() + om.abs()) + (l + om - 1.0).abs()) * a.abs()).all()
    ops.check_status()


def test_mix_unmixed_rows_are_copies_whatever_the_partner_holds():
    x = torch.randn(6, 64, 96)
    x[1, 3, 5], x[3, 0, 0], x[5, 63, 95] = float("inf"), float("nan"), -float("inf")
    perm = torch.tensor([1, 3, 5, 0, 2, 4])
    lam = torch.tensor([1.0, 1.0, 1.0, 0.5, 0.25, 1.0])
    out = train_ops.mix_features(x.to(DEV), perm.to(DEV), lam.to(DEV)).cpu()
    for b in (0, 1, 2, 5):
        assert torch.equal(out[b].view(torch.int32), x[b].view(torch.int32)), b
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[2]).all() and torch.isfinite(out[4]).all()
    ops.check_status()


def test_mix_bad_arguments():
    x = torch.randn(4, 64, 96, device=DEV)
    lam = torch.full((4,), 0.5, device=DEV)
    out = train_ops.mix_features(x, torch.tensor([1, 4, 3, -1], device=DEV), lam)
    assert (out[1] == 0).all() and (out[3] == 0).all() and not (out[0] == 0).all()
    with pytest.raises(_native.SirError):
        ops.check_status()
    with pytest.raises(_native.SirError):                                   # t % 4 != 0
        train_ops.mix_features(torch.randn(4, 64, 98, device=DEV), torch.arange(4, device=DEV), lam)
    lib = _native.lib()
    perm = torch.arange(4, device=DEV)
    rc = lib.sir_mix_features(get_featurizer().handle, x.data_ptr(), perm.data_ptr(), lam.data_ptr(), 4, 64, 96, x.data_ptr(),
                              _native.current_stream_ptr())
    assert rc == -1                                                         # out aliases x
    ops.check_status()


# ---- 3. norm ---------------------------------------------------------------------------------------------------------
def _norm_bound(norm):
    """One partial: per thread a chain of 16 fmas (the square is not rounded on its own), then a binary tree of depth 8
    in LDS -- every addend is >= 0, so the partial's relative error is <= gamma_24 = 24u / (1 - 24u).  The partials are
    summed in double (their 2^-53 roundings are below fp32 resolution: one more u covers them and the conversion of
    the square root's argument), the square root halves the relative error, the result is rounded to fp32 once."""
    g24 = 24 * U / (1 - 24 * U)
    return ((1 + g24) ** 0.5 - 1 + 2 * U) * norm


def _f64_norm(grads):
    return torch.sqrt(sum((g.detach().cpu().double() ** 2).sum() for g in grads)).item()


def _backward(sd, bsz):
    m = _model(sd)
    x = synth.synth_features(bsz, 200, seed=bsz).to(DEV)
    y = synth.synth_labels(bsz, 31, seed=bsz + 1).to(DEV)
    train_ops.fused_cross_entropy(m(x), y).backward()
    return m


def _synthetic_params(scale=1.0):
    g = torch.Generator().manual_seed(11)
    ps = [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in (1, 5, 4095, 4097, 70001, 8192)]
    for p in ps:
        p.grad = (torch.randn(p.numel(), generator=g) * scale).to(DEV)
    return ps


@pytest.mark.parametrize("which", ["model8", "model256", "synthetic"])
def test_grad_norm_vs_float64_and_repeatable(sd, which):
    params = _synthetic_params() if which == "synthetic" else list(_backward(sd, 8 if which == "model8" else 256).parameters())
    assert which == "synthetic" or len(params) == 29
    ref = _f64_norm([p.grad for p in params])
    before = [p.grad.clone() for p in params]
    norms = [train_ops.clip_grad_norm_(params, 1e30) for _ in range(3)]          # far above: coef == 1
    print(f"grad norm {which}: device {norms[0].item():.9g} float64 {ref:.9g} err {abs(norms[0].item() - ref):.3e} "
          f"bound {_norm_bound(ref):.3e}")
    assert abs(float(norms[0].double()) - ref) <= _norm_bound(ref)
    assert torch.equal(norms[0], norms[1]) and torch.equal(norms[0], norms[2])
    for p, b in zip(params, before):
        assert torch.equal(p.grad, b)                                            # norm < max_norm: bit-unchanged
    ops.check_status()


def _raw_clip(grads, max_norm, in_place=1):
    lib, h = _native.lib(), get_featurizer().handle
    G, N = train_ops._grad_arrays(grads)
    n = lib.sir_grad_norm_partials(len(grads), N)
    part = torch.empty(n, device=DEV)
    out2 = torch.empty(2, device=DEV)
    rc = lib.sir_grad_norm(h, len(grads), G, N, max_norm, part.data_ptr(), n, out2.data_ptr(), in_place, _native.current_stream_ptr())
    return rc, out2, part


def test_clip_scales_by_the_coefficient_it_reports(sd):
    m = _backward(sd, 8)
    params = list(m.parameters())
    m.fc.bias.grad = None                                                        # a frozen parameter is left out
    grads = [p.grad for p in params if p.grad is not None]
    before = [g.clone() for g in grads]
    ref = _f64_norm(before)
    max_norm = 0.25 * ref
    rc, out2, part = _raw_clip(grads, max_norm)
    assert rc == 0
    total, coef = out2.tolist()
    assert abs(total - ref) <= _norm_bound(ref)
    assert coef == np.float32(max_norm) / (np.float32(total) + np.float32(1e-6)) and coef < 1.0
    assert part.numel() == sum((g.numel() + 4095) // 4096 for g in grads)
    for g, b in zip(grads, before):
        assert torch.equal(g, b * out2[1])                                       # g * coef, one fp32 rounding
    # the wrapper: same norm bits from the same gradients, frozen parameter untouched
    for g, b in zip(grads, before):
        g.copy_(b)
    norm = train_ops.clip_grad_norm_(params, max_norm)
    assert norm.item() == total and m.fc.bias.grad is None
    # without the in-place flag nothing is scaled
    for g, b in zip(grads, before):
        g.copy_(b)
    rc, out2b, _ = _raw_clip(grads, max_norm, in_place=0)
    assert rc == 0 and torch.equal(out2b, out2)
    for g, b in zip(grads, before):
        assert torch.equal(g, b)
    ops.check_status()


def test_clip_with_a_non_finite_gradient_behaves_as_torch():
    params = _synthetic_params()
    params[3].grad[100] = float("inf")
    cpu = [torch.nn.Parameter(torch.zeros(p.numel())) for p in params]
    for c, p in zip(cpu, params):
        c.grad = p.grad.cpu().clone()
    ref_norm = torch.nn.utils.clip_grad_norm_(cpu, 1.0)
    norm = train_ops.clip_grad_norm_(params, 1.0)
    assert torch.isinf(ref_norm).item() and torch.isinf(norm).item()
    for c, p in zip(cpu, params):
        assert torch.equal(torch.isnan(c.grad), torch.isnan(p.grad.cpu()))
        assert torch.equal(torch.nan_to_num(c.grad), torch.nan_to_num(p.grad.cpu()))
    assert not torch.isfinite(params[3].grad).all()
    ops.check_status()


def test_clip_bad_arguments():
    params = _synthetic_params()
    grads = [p.grad for p in params]
    for bad in (0.0, -1.0, float("nan")):
        assert _raw_clip(grads, bad)[0] == -1
    too_many = [torch.nn.Parameter(torch.zeros(3, device=DEV)) for _ in range(33)]
    for p in too_many:
        p.grad = torch.ones(3, device=DEV)
    with pytest.raises(_native.SirError):
        train_ops.clip_grad_norm_(too_many, 1.0)
    ops.check_status()


# ---- 4. clipped Adam -------------------------------------------------------------------------------------------------
def _adam_setup(max_grad_norm):
    torch.manual_seed(0)
    ps = [torch.randn(n) for n in (5, 4097, 70000)]
    gs = [[torch.randn_like(p) * (10.0 ** (-i)) for p in ps] for i in range(3)]
    dev_ps = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps]
    opt = FusedAdam(dev_ps, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=max_grad_norm)
    return ps, gs, dev_ps, opt


def _state(opt):
    gs = next(iter(opt.state.values()))
    return gs["exp_avg"], gs["exp_avg_sq"]


def test_clipped_adam_equals_clip_then_adam_bit_for_bit():
    max_norm = 20.0                                   # norms of the three steps: ~272, ~27, ~2.7 -> clipped, clipped, not
    ps, gs, pa, oa = _adam_setup(None)
    _, _, pb, ob = _adam_setup(max_norm)
    coefs = []
    for step in range(3):
        for p, q, g in zip(pa, pb, gs[step]):
            p.grad, q.grad = g.to(DEV), g.to(DEV)
        norm = train_ops.clip_grad_norm_(pa, max_norm)
        oa.step()
        ob.step()
        assert ob.last_grad_norm[0].item() == norm.item()
        coefs.append(ob.last_grad_norm[1].item())
        for q, g in zip(pb, gs[step]):
            assert torch.equal(q.grad.cpu(), g)                              # the fused form leaves .grad unscaled
        for p, q in zip(pa, pb):
            assert torch.equal(p, q)
        for a, b in zip(_state(oa), _state(ob)):
            assert torch.equal(a, b)
    assert coefs[0] < 1.0 and coefs[1] < 1.0 and coefs[2] == 1.0, coefs
    ops.check_status()


def test_max_grad_norm_far_above_is_the_plain_step():
    ps, gs, pa, oa = _adam_setup(None)
    _, _, pb, ob = _adam_setup(1e30)
    for step in range(3):
        for p, q, g in zip(pa, pb, gs[step]):
            p.grad, q.grad = g.to(DEV), g.to(DEV)
        oa.step()
        ob.step()
    assert ob.last_grad_norm[1].item() == 1.0
    for p, q in zip(pa, pb):
        assert torch.equal(p, q)
    for a, b in zip(_state(oa), _state(ob)):
        assert torch.equal(a, b)
    ops.check_status()


def test_clipped_adam_vs_torch_float64():
    """clip_grad_norm_ + torch.optim.Adam in float64, the bound of test_adam_kernel_vs_oracle_over_steps (2e-6)."""
    max_norm = 20.0
    ps, gs, dev_ps, opt = _adam_setup(max_norm)
    ref_ps = [torch.nn.Parameter(p.double().clone()) for p in ps]
    ref_opt = torch.optim.Adam(ref_ps, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for step in range(3):
        for p, r, g in zip(dev_ps, ref_ps, gs[step]):
            p.grad, r.grad = g.to(DEV), g.double().clone()
        opt.step()
        torch.nn.utils.clip_grad_norm_(ref_ps, max_norm)
        ref_opt.step()
    for p, r in zip(dev_ps, ref_ps):
        assert (p.detach().cpu().double() - r.detach()).abs().max() < 2e-6
    ops.check_status()


# ---- 5. whole steps --------------------------------------------------------------------------------------------------
STEPS = 3
EPS = 0.1
MIX = [(0.7, [3, 0, 1, 2, 7, 6, 5, 4]), (0.35, [1, 2, 3, 4, 5, 6, 7, 0]), (0.9, [7, 6, 5, 4, 3, 2, 1, 0])]


def _ref_loss(m, x, y, lam, perm):
    lamt = torch.full((x.shape[0],), lam, dtype=torch.float64)
    logits = m(recipe_ref.mix(x, torch.tensor(perm), lamt))
    yb = y[torch.tensor(perm)]
    return lam * F.cross_entropy(logits, y, label_smoothing=EPS) + (1 - lam) * F.cross_entropy(logits, yb, label_smoothing=EPS)


def test_three_recipe_steps_match_torch_float64(sd):
    """The configuration of test_ten_step_trajectory_matches_reference_golden (same batch, dropout off, same lr / wd), three
    steps with a fixed (lam, perm) per step, label smoothing 0.1 and max_norm = half the reference's first-step norm,
    against TrainRef in float64 fed recipe_ref.mix(x), the two-term loss, clip_grad_norm_ and torch.optim.Adam.
    Bounds as in that test: loss 1e-4 per step, sampled parameters 0.9-quantile 2e-6 K and max 2.1 lr K, BN statistics
    rtol 1e-4 K / atol 5e-6 K."""
    inp = cases.model_inputs()
    x, y = inp["x_train8"], inp["y_train8"]
    k = STEPS
    sd64 = {n: (v.double() if v.is_floating_point() else v) for n, v in sd.items()}

    def ref_model():
        r = model_ref.TrainRef(sd, 31).double().train()
        r.load_state_dict(sd64)
        r.gru.dropout = 0.0
        return r

    probe = ref_model()
    _ref_loss(probe, x.double(), y, *MIX[0]).backward()
    max_norm = 0.5 * _f64_norm([p.grad for p in probe.parameters()])

    ref = ref_model()
    ropt = torch.optim.Adam(ref.parameters(), lr=cases.LR, weight_decay=cases.WEIGHT_DECAY)
    ref_losses, ref_norms = [], []
    for lam, perm in MIX:
        ropt.zero_grad(set_to_none=True)
        loss = _ref_loss(ref, x.double(), y, lam, perm)
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm).item()
        assert max_norm / (norm + 1e-6) < 1.0, "mis-configured: the reference run does not clip on this step"
        ropt.step()
        ref_losses.append(loss.item())
        ref_norms.append(norm)

    m = _model(sd)
    opt = FusedAdam(m.parameters(), lr=cases.LR, weight_decay=cases.WEIGHT_DECAY, max_grad_norm=max_norm)
    xd, yd = x.to(DEV), y.to(DEV)
    losses, norms = [], []
    for lam, perm in MIX:
        permd = torch.tensor(perm, device=DEV)
        lamd = torch.full((8,), lam, device=DEV)
        opt.zero_grad(set_to_none=True)
        loss = train_ops.fused_cross_entropy(m(train_ops.mix_features(xd, permd, lamd)), yd, yd[permd], lamd, label_smoothing=EPS)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        norms.append(opt.last_grad_norm.tolist())
    torch.cuda.synchronize()
    dl = np.abs(np.asarray(losses) - np.asarray(ref_losses))
    print("recipe steps: losses", losses, "reference", ref_losses, "max diff", dl.max())
    print("recipe steps: {norm, coef}", norms, "reference norms", ref_norms, "max_norm", max_norm)
    assert dl.max() <= 1e-4, dl
    assert all(c < 1.0 for _, c in norms)
    worst = 0.0
    rparams = dict(ref.named_parameters())
    for name, p in m.named_parameters():
        flat = p.detach().cpu().flatten()
        idx = cases.sample_indices(name, flat.numel())
        d = np.abs(flat[idx].double().numpy() - rparams[name].detach().flatten()[idx].numpy())
        worst = max(worst, float(d.max()))
        assert np.quantile(d, 0.9) <= 2e-6 * k and d.max() <= 2.1 * cases.LR * k, (name, np.quantile(d, 0.9), d.max())
    print("recipe steps: worst sampled parameter difference after", k, "steps:", worst)
    for i in (1, 2, 3):
        bn, rbn = getattr(m, f"bn{i}"), getattr(ref, f"bn{i}")
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), rbn.running_mean.numpy(), rtol=1e-4 * k, atol=5e-6 * k)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), rbn.running_var.numpy(), rtol=1e-4 * k, atol=5e-6 * k)
    ops.check_status()


# ---- 6. entry points -------------------------------------------------------------------------------------------------
def test_train_epoch_with_the_recipe_matches_inline_steps(sd):
    from sir_amd.feature_store import FeatureStore
    from sir_amd.scripts.train import train_epoch
    n, bsz = 22, 6                                           # (the last batch is ragged: 4 items)
    feats = synth.synth_features(n, 200, seed=9).to(DEV)
    labels = synth.synth_labels(n, 31, seed=10).to(DEV)
    store = FeatureStore.from_tensors(feats, [200] * n, labels)
    kw = dict(shuffle=True, seed=3, epoch=1, augment_prob=0.5)

    ma = _model(sd)
    oa = FusedAdam(ma.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    mx = train_ops.Mixup(0.2, seed=5)
    ref_losses = []
    for mel, label in store.epoch_batches(bsz, **kw):
        perm, lam = mx.draw(mel.shape[0])
        perm, lam = perm.to(DEV), lam.to(DEV)
        oa.zero_grad(set_to_none=True)
        loss = train_ops.fused_cross_entropy(ma(train_ops.mix_features(mel, perm, lam)), label, label[perm], lam, label_smoothing=0.1)
        loss.backward()
        oa.step()
        ref_losses.append(loss.detach())
    ref_mean = torch.stack(ref_losses).mean().item()

    mb = _model(sd)
    ob = FusedAdam(mb.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    mean = train_epoch(mb, store.epoch_batches(bsz, **kw), ob, torch.nn.CrossEntropyLoss(label_smoothing=0.1), DEV,
                       mixup=train_ops.Mixup(0.2, seed=5))
    torch.cuda.synchronize()
    assert mean == ref_mean
    assert torch.equal(oa.last_grad_norm, ob.last_grad_norm)
    for (name, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(pa, pb), name
    ops.check_status()


def test_waveform_epoch_with_the_recipe_matches_inline_steps(sd):
    from sir_amd.scripts.train import train_epoch_waveforms
    nb, bsz = 3, 6
    waves = [(synth.synth_clips(bsz, 30000 + 1000 * i, seed=60 + i) * 32767).round().to(torch.int16) for i in range(nb)]
    lens = [torch.tensor([w.shape[1] - 37 * j for j in range(bsz)], dtype=torch.int32) for w in waves]
    labels = [synth.synth_labels(bsz, 31, seed=70 + i) for i in range(nb)]

    ma = _model(sd)
    oa = FusedAdam(ma.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    mx = train_ops.Mixup(0.2, seed=6)
    fz = get_featurizer()
    ref_losses = []
    for w, l, y in zip(waves, lens, labels):
        x, y = fz(w.to(DEV), l.to(DEV), t_pad=200), y.to(DEV)
        perm, lam = mx.draw(bsz)
        perm, lam = perm.to(DEV), lam.to(DEV)
        oa.zero_grad(set_to_none=True)
        loss = train_ops.fused_cross_entropy(ma(train_ops.mix_features(x, perm, lam)), y, y[perm], lam, label_smoothing=0.1)
        loss.backward()
        oa.step()
        ref_losses.append(loss.detach())
    ref_mean = torch.stack(ref_losses).mean().item()

    mb = _model(sd)
    ob = FusedAdam(mb.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    mean = train_epoch_waveforms(mb, list(zip(waves, lens, labels)), ob, torch.nn.CrossEntropyLoss(label_smoothing=0.1), DEV,
                                 mixup=train_ops.Mixup(0.2, seed=6))
    torch.cuda.synchronize()
    assert mean == ref_mean
    for (name, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(pa, pb), name
    ops.check_status()


def test_train_with_the_three_yaml_keys_runs_to_a_checkpoint(tmp_path):
    from sir_amd.scripts import precompute_features as pf
    from sir_amd.scripts import train as tr
    from test_pipeline_gpu import LABELS, _make_corpus

    rows = _make_corpus(str(tmp_path / "wav"))
    csvs = {}
    for split, sl in (("train", slice(0, 16)), ("valid", slice(16, 20))):
        p = tmp_path / f"{split}_data.csv"
        pd.DataFrame(rows[sl]).to_csv(p, index=False)
        csvs[split] = str(p)
        pf.precompute_dataset_features(str(p), str(tmp_path / "cache"))
    lm = tmp_path / "label_map.json"
    lm.write_text(json.dumps({l: i for i, l in enumerate(sorted(LABELS))}))
    cfg = {"batch_size": 8, "num_workers": 0, "num_labels": 31, "lr": 1e-3, "weight_decay": 1e-4, "epochs": 2,
           "early_stop_patience": 5, "augment_prob": 0.7, "cache_dir": str(tmp_path / "cache"), "use_feature_cache": True,
           "save_path": str(tmp_path / "ckpt"), "mixup": 0.2, "label_smoothing": 0.1, "clip_grad_norm": 1.0}
    args = types.SimpleNamespace(train_csv=csvs["train"], val_csv=csvs["valid"], label_map=str(lm))
    best = tr.train(args, cfg)
    assert 0.0 <= best <= 1.0
    best_fused = tr.train(args, dict(cfg, fused_features=True, epochs=1, save_path=str(tmp_path / "ckpt_fused")))
    assert 0.0 <= best_fused <= 1.0
    if best > 0:                                          # the reference only saves on improvement over 0 (train.py:281)
        sd_ck = torch.load(os.path.join(cfg["save_path"], "best_model.pt"))
        assert list(sd_ck.keys()) == list(synth.synth_state_dict(31).keys())
        assert all(torch.isfinite(v).all() for v in sd_ck.values() if v.is_floating_point())
    ops.check_status()
