"""The training step differentiated with respect to its input features (``sir_model_train_bwd_x``,
``conv1_bwd_data_kernel``) and ``sir_amd.explain`` on top of it.

Reference and bound: ``tests/input_grad_ref.py`` -- ``oracle.model_ref.forward`` in float64, differentiated with
``torch.autograd.grad`` at the device's forward values; ``max |a - b| <= 2e-3 * rms(dx)``, loss 1e-5, logits 2e-5.  Every test
prints the ratio it measured and ends in ``ops.check_status()``.
"""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import cases
import host_rng
import input_grad_ref as ref
from sir_amd import _native, explain, finetune, ops, synth, train_ops
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEW_ID = "bwd_conv1_dgrad"
WGRAD_IDS = ("bwd_gru_dw_l1", "bwd_gru_dw_l0", "bwd_conv3_wgrad", "bwd_conv2_wgrad")
DGRAD_IDS = ("bwd_gru_dx_l1", "bwd_gru_dx_l0", "bwd_conv3_dgrad", "bwd_conv2_dgrad", NEW_ID)


@pytest.fixture(scope="module")
def sd():
    return synth.synth_state_dict(31, seed=0)


def _model(sd, frozen_bn=(), dropout=0.0):
    m = CNNAudioGRU(31)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.gru.dropout = dropout
    for i in frozen_bn:
        getattr(m, f"bn{i}").eval()
    return m


def _step(m, x, y, x_grad=True):
    """One forward / backward of the training path; returns (logits, loss, x.grad or None)."""
    m.zero_grad(set_to_none=True)
    xd = x.to(DEV).requires_grad_(x_grad)
    logits = m(xd)
    loss = train_ops.fused_cross_entropy(logits, y.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), loss.detach(), xd.grad


def _check_step(tag, sd, m, x, y, logits, loss, dx, bn_frozen=(False, False, False), dropout_mask=None):
    bsz, t = x.shape[0], x.shape[-1]
    zo, yo = ref.device_forward_values(m, sd, x, bsz, t)
    ref_loss, ref_logits, ref_dx = ref.reference(sd, x, zo, yo, labels=y, bn_frozen=bn_frozen, dropout_mask=dropout_mask)
    r = ref.ratio(dx, ref_dx)
    print(f"{tag}: max|dx - ref| / rms(ref) = {r:.2e} (rms {ref_dx.pow(2).mean().sqrt().item():.2e}), loss err "
          f"{abs(loss.item() - ref_loss.item()):.1e}, logits err {(logits.cpu().double() - ref_logits).abs().max().item():.1e}")
    assert abs(loss.item() - ref_loss.item()) < 1e-5
    assert (logits.cpu().double() - ref_logits).abs().max() < 2e-5
    assert r <= ref.GRAD_BOUND, (tag, r)


@pytest.mark.parametrize("bsz,t,four_d", [(5, 200, False), (18, 96, True)])
def test_x_grad_live_bn_vs_oracle(sd, bsz, t, four_d):
    """Live statistics, no dropout: partial GRU groups, several column tiles of the data-gradient kernel (the last one
    partial), image edges on all four sides.  The 4-D case gets its gradient in the 4-D shape."""
    x = cases.varied_features(bsz, t, seed=900 + bsz)
    y = synth.synth_labels(bsz, 31, seed=901 + bsz)
    xin = x.unsqueeze(1) if four_d else x
    m = _model(sd)
    logits, loss, dx = _step(m, xin, y)
    assert dx is not None and dx.shape == xin.shape and dx.is_contiguous()
    _check_step(f"live B={bsz} T={t}", sd, m, x, y, logits, loss, dx)
    ops.check_status()


def test_x_grad_with_dropout_vs_oracle(sd):
    bsz, t, s, p = 3, 200, 25, 0.5
    x = cases.varied_features(bsz, t, seed=910)
    y = synth.synth_labels(bsz, 31, seed=911)
    m = _model(sd, dropout=p)
    logits, loss, dx = _step(m, x, y)
    seed, p_used = m._sir_last_dropout
    assert p_used == p
    keep = torch.from_numpy(host_rng.dropout_keep(seed, bsz * s * 512, p)).view(bsz, s, 512)
    _check_step("dropout 0.5", sd, m, x, y, logits, loss, dx, dropout_mask=keep.float() / (1.0 - p))
    ops.check_status()


@pytest.mark.parametrize("frozen_bn", [(1,), (1, 2, 3)])
def test_x_grad_frozen_bn_vs_oracle(sd, frozen_bn):
    """bn1 on its running statistics (the affine dz branch; with every conv1 / bn1 gradient still wanted the reduce pass runs
    beside it), bn2 / bn3 live or frozen too."""
    bsz, t = 5, 200
    x = cases.varied_features(bsz, t, seed=920)
    y = synth.synth_labels(bsz, 31, seed=921)
    m = _model(sd, frozen_bn=frozen_bn)
    logits, loss, dx = _step(m, x, y)
    _check_step(f"frozen bn{frozen_bn}", sd, m, x, y, logits, loss, dx, bn_frozen=tuple(i in frozen_bn for i in (1, 2, 3)))
    ops.check_status()


def test_explain_input_gradient_on_eval_model(sd):
    bsz, t = 4, 200
    x = cases.varied_features(bsz, t, seed=930)
    target = torch.tensor([3, 30, 0, 17])
    m = _model(sd).eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    flags = {n: mod.training for n, mod in m.named_modules()}
    step = train_ops.dropout_step()
    xd = x.to(DEV)
    logits, dx = explain.input_gradient(m, xd, target.to(DEV))
    torch.cuda.synchronize()
    assert dx.shape == xd.shape and not dx.requires_grad and not xd.requires_grad
    zo, yo = ref.device_forward_values(m, sd, x, bsz, t)
    _, ref_logits, ref_dx = ref.reference(sd, x, zo, yo, target=target, bn_frozen=(True, True, True))
    r = ref.ratio(dx, ref_dx)
    with torch.no_grad():
        eval_logits = m(xd)
    print(f"explain.input_gradient: max|dx - ref| / rms(ref) = {r:.2e}, logits vs eval "
          f"{(logits - eval_logits).abs().max().item():.1e}, vs oracle {(logits.cpu().double() - ref_logits).abs().max().item():.1e}")
    assert r <= ref.GRAD_BOUND
    assert (logits - eval_logits).abs().max() < 2e-5
    for k, v in before.items():                              # parameters, running statistics, num_batches_tracked
        assert torch.equal(m.state_dict()[k], v), k
    assert all(p.grad is None for p in m.parameters())
    assert {n: mod.training for n, mod in m.named_modules()} == flags
    assert train_ops.dropout_step() == step
    # clip 0 on its own: the same gradient (frozen statistics: the rows of a batch do not see each other)
    _, dx0 = explain.input_gradient(m, xd[:1], target[:1].to(DEV))
    r0 = ref.ratio(dx0[0], ref_dx[0])
    print(f"clip 0 alone: {r0:.2e}")
    assert r0 <= ref.GRAD_BOUND
    # a model in train() mode with gradients already in place: the same result, .grad untouched; default target = argmax
    m.train()
    _step(m, x, synth.synth_labels(bsz, 31, seed=931), x_grad=False)
    grads = {n: p.grad for n, p in m.named_parameters()}
    kept = {n: g.clone() for n, g in grads.items()}
    stats = {k: v.clone() for k, v in m.state_dict().items()}
    logits2, dx2 = explain.input_gradient(m, xd)
    sal = explain.saliency(m, xd)
    torch.cuda.synchronize()
    assert m.training and m.bn1.training
    for n, p in m.named_parameters():
        assert p.grad is grads[n] and torch.equal(p.grad, kept[n]), n
    for k, v in stats.items():
        assert torch.equal(m.state_dict()[k], v), k
    assert sal.shape == (bsz, 64, t) and torch.equal(sal, (dx2 * xd).abs())
    ops.check_status()


def _c_backward(m, x, dlogits, fn_name, dfeats=None):
    """One direct C call of the backward on the workspace ``m``'s last forward left, all 29 gradients into a buffer of its own."""
    lib, h = _native.lib(), get_featurizer().handle
    buf = train_ops.GradBuffer(m)
    w, _keep = ops.cached_weights(m)
    seed, p = m._sir_last_dropout
    ws = m._sir_train["ws"].buf
    args = [h, C.byref(w), x.data_ptr(), dlogits.data_ptr(), x.shape[0], x.shape[-1], p, seed, C.byref(train_ops.bn_config(m)),
            C.byref(buf.struct)]
    if fn_name == "sir_model_train_bwd_x":
        args.append(dfeats.data_ptr() if dfeats is not None else None)
    args += [ws.data_ptr(), ws.numel(), _native.BWD_ALL, _native.current_stream_ptr()]
    _native.check(getattr(lib, fn_name)(*args), fn_name)
    torch.cuda.synchronize()
    return buf.flat


def test_nothing_existing_moves(sd):
    """All 29 parameter gradients bit-identical whether or not the input gradient is asked for, and
    ``sir_model_train_bwd_x(dfeats = NULL)`` against ``sir_model_train_bwd_cfg``; the ordinary step never launches the new kernel."""
    bsz, t = 21, 200
    x = cases.varied_features(bsz, t, seed=940)
    y = synth.synth_labels(bsz, 31, seed=941)
    ma, mb = _model(sd), _model(sd)
    _step(ma, x, y, x_grad=False)
    _, _, dx = _step(mb, x, y, x_grad=True)
    assert dx is not None and dx.abs().max() > 0
    for (n, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    counts, _ = ref.launch_counts(lambda: _step(ma, x, y, x_grad=False))
    print("ordinary step:", NEW_ID, counts[NEW_ID], "bwd_conv1", counts["bwd_conv1"])
    assert counts[NEW_ID] == 0 and counts["bwd_conv1"] == 1
    counts_b, _ = ref.launch_counts(lambda: _step(mb, x, y, x_grad=True))
    assert counts_b[NEW_ID] == 1
    # the C calls, on the workspace of ma's last forward
    xd = x.to(DEV)
    logits = ma(xd)
    dlogits = torch.empty_like(logits)
    loss = torch.empty((), device=DEV)
    _native.check(_native.lib().sir_ce_loss(get_featurizer().handle, logits.data_ptr(), y.to(DEV).data_ptr(), bsz, 31, loss.data_ptr(),
                                            dlogits.data_ptr(), 1.0, _native.current_stream_ptr()), "sir_ce_loss")
    g_cfg = _c_backward(ma, xd, dlogits, "sir_model_train_bwd_cfg")
    g_null = _c_backward(ma, xd, dlogits, "sir_model_train_bwd_x", None)
    dfeats = torch.empty_like(xd)
    g_x = _c_backward(ma, xd, dlogits, "sir_model_train_bwd_x", dfeats)
    assert g_cfg.abs().max() > 0
    assert torch.equal(g_cfg, g_null) and torch.equal(g_cfg, g_x)
    assert torch.equal(dfeats, dx)
    ops.check_status()


def test_input_gradient_alone_prunes_every_weight_gradient(sd):
    bsz, t = 21, 200
    x = cases.varied_features(bsz, t, seed=950)
    y = synth.synth_labels(bsz, 31, seed=951)
    _, _, dx_full = _step(_model(sd), x, y)
    m = _model(sd)
    for p in m.parameters():
        p.requires_grad_(False)
    for rep in range(2):                                     # two-stream form
        _, _, dx = _step(m, x, y)
        assert torch.equal(dx, dx_full), rep
    out = {}
    counts, _ = ref.launch_counts(lambda: out.update(dx=_step(m, x, y)[2]))
    assert torch.equal(out["dx"], dx_full)                   # one-stream form
    assert all(p.grad is None for p in m.parameters())
    print("input gradient alone, launches:", {k: counts[k] for k in WGRAD_IDS + DGRAD_IDS + ("bwd_conv1",)})
    for k in WGRAD_IDS:
        assert counts[k] == 0, k
    for k in DGRAD_IDS:
        assert counts[k] > 0, k
    # frozen statistics on top: conv1's reduce pass has nothing left to feed
    mf = _model(sd, frozen_bn=(1, 2, 3))
    _, _, dxf_full = _step(mf, x, y)
    for p in mf.parameters():
        p.requires_grad_(False)
    counts, _ = ref.launch_counts(lambda: out.update(dx=_step(mf, x, y)[2]))
    assert torch.equal(out["dx"], dxf_full)
    assert counts["bwd_conv1"] == 0 and counts[NEW_ID] == 1
    ops.check_status()


def test_split_backward_writes_the_same_input_gradient(sd, monkeypatch):
    """SIR_BWD_HEAD_GRU then SIR_BWD_CNN with dfeats == SIR_BWD_ALL, with every conv / BatchNorm parameter frozen so that the
    exchange code would leave the second half out (``cnn=False``): the one-rank gloo idiom of
    ``test_train_gpu.py::test_backward_in_two_halves_is_bit_identical``."""
    import torch.distributed as dist
    bsz, t = 5, 200
    x = cases.varied_features(bsz, t, seed=960)
    y = synth.synth_labels(bsz, 31, seed=961)

    def run():
        m = _model(sd)
        finetune.freeze(m, {"cnn"})
        return m, _step(m, x, y)[2]

    m0, dx0 = run()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29657")
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        monkeypatch.setattr(train_ops, "world_size", lambda: 2)          # take the two-bucket branch
        monkeypatch.setattr(train_ops, "OVERLAP_GRAD_EXCHANGE", True)
        parts, lib = [], _native.lib()
        real = lib.sir_model_train_bwd_emb               # (the one backward the node calls; `part` is argument 15 of its 17)
        monkeypatch.setattr(lib, "sir_model_train_bwd_emb", lambda *a: parts.append(a[15]) or real(*a))
        m1, dx1 = run()
        assert parts == [_native.BWD_HEAD_GRU, _native.BWD_CNN]
        assert torch.equal(dx1, dx0)
        for (n, p), (_, q) in zip(m0.named_parameters(), m1.named_parameters()):
            if n.startswith(("conv", "bn")):
                assert p.grad is None and q.grad is None, n
            else:                                            # (sum over one rank, then the patched 1 / 2)
                assert torch.equal(q.grad * 2.0, p.grad), n
    finally:
        dist.destroy_process_group()
    ops.check_status()


def test_fgsm_raises_the_loss_by_steps_of_eps(sd):
    bsz, t, eps = 8, 200, 1e-2
    x = cases.varied_features(bsz, t, seed=970).to(DEV)
    y = synth.synth_labels(bsz, 31, seed=971).to(DEV)
    m = _model(sd).eval()
    x_adv = explain.fgsm(m, x, y, eps)
    with torch.no_grad():
        ce, ce_adv = F.cross_entropy(m(x), y).item(), F.cross_entropy(m(x_adv), y).item()
    print(f"fgsm eps={eps}: CE {ce:.6f} -> {ce_adv:.6f}")
    assert ce_adv > ce
    # x + eps * sign(dx) is rounded to float32 (eps once, the sum once): |x_adv - x| is eps within one spacing of x_adv wherever dx != 0, and 0
    # elsewhere
    step = (x_adv.double() - x.double()).abs()
    moved = step > 0
    spacing = torch.maximum(x_adv.abs(), x.abs()).double() * 2.0 ** -23
    assert moved.float().mean() > 0.99
    assert ((step - eps).abs()[moved] <= spacing[moved] + eps * 2.0 ** -24).all()
    assert abs(step.max().item() - eps) <= spacing.max().item() + eps * 2.0 ** -24
    assert torch.equal(explain.fgsm(m, x, y, 0.0), x)
    ops.check_status()
