"""Shared pieces of the ragged-gradient tests (``test_ragged_grad_host.py``, ``test_ragged_grad_gpu.py``).

The function: row b of the logits is ``model_ref.forward(sd, x[b:b+1, :, :frames[b]], train=False, dropout_mask=...)`` -- every
BatchNorm on its running statistics, the inter-layer dropout mask of the dense step for ``t < S_b``, the attention softmax over
``t < S_b`` -- and the loss is the mean cross-entropy over the rows.

``per_clip_reference``: that statement, clip by clip, in float64 under ``torch.autograd``; with ``zo`` / ``yo`` it is evaluated at
the device's forward values sliced to each clip's widths (``input_grad_ref.device_forward_values``), so that no ReLU / pool tie
can route differently and no element is excluded.

``masked_dense``: the masked dense form a kernel chain can implement, restated in this file's own code (float64): feature columns
``>= frames[b]`` count as zero, each block's pooled map is zero at and beyond the clip's new width, a GRU step ``t >= S_b`` holds
``h`` (so the reverse direction starts at ``S_b - 1`` from 0), attention scores at ``t >= S_b`` are -inf.

Bounds are the project's own: gradients ``max |a - ref| <= 2e-3 * rms(ref)``, logits 2e-5, loss 1e-5; a gradient whose reference
maximum is <= 1e-7 (``attention.bias``: analytically zero by the softmax's shift invariance) is skipped.
"""
import torch
import torch.nn.functional as F

from oracle import model_ref

GRAD_BOUND = 2e-3
LOGIT_BOUND = 2e-5
LOSS_BOUND = 1e-5
SKIP_BELOW = 1e-7
CASE_FRAMES = [40, 8, 9, 15, 17, 23, 31, 39, 16, 25]          # S_b = 1, an odd width at every stage (15 -> 7 -> 3 -> 1), a full-width clip


def _d(v):
    return v.double() if torch.is_tensor(v) and v.is_floating_point() else v


def _leaves(sd):
    params = {k: sd[k].detach().double().clone().requires_grad_(True) for k in model_ref.PARAM_KEYS}
    full = {k: _d(v) for k, v in sd.items()}
    full.update(params)
    return params, full


def per_clip_reference(sd, x, frames, labels, zo=None, yo=None, dropout_mask=None):
    """float64 -> (loss, logits [B, C], {parameter: gradient}, dx [B, 64, T]).  ``dropout_mask`` [B, S, 512] is read for
    ``t < S_b`` only; columns of ``x`` at or beyond ``frames[b]`` are not read at all."""
    bsz, t = x.shape[0], x.shape[-1]
    params, full = _leaves(sd)
    xs = []
    rows = []
    for b, f in enumerate(frames):
        xb = x[b].detach().cpu().double().view(64, t)[None, :, :f].clone().requires_grad_(True)
        xs.append(xb)
        w = {1: f, 2: f // 2, 3: f // 4}
        zb = {i: _d(zo[i][b:b + 1, :, :, :w[i]]) for i in w} if zo is not None else None
        yb = {i: _d(yo[i][b:b + 1, :, :, :w[i]]) for i in w} if yo is not None else None
        mb = _d(dropout_mask[b:b + 1, :f // 8]) if dropout_mask is not None else None
        rows.append(model_ref.forward(full, xb, train=False, dropout_mask=mb, z_override=zb, y_override=yb))
    logits = torch.cat(rows, 0)
    loss = F.cross_entropy(logits, labels)
    grads = torch.autograd.grad(loss, [params[k] for k in model_ref.PARAM_KEYS] + xs)
    dx = torch.zeros(bsz, 64, t, dtype=torch.float64)
    for b, (f, g) in enumerate(zip(frames, grads[len(model_ref.PARAM_KEYS):])):
        dx[b, :, :f] = g[0]
    return loss.detach(), logits.detach(), dict(zip(model_ref.PARAM_KEYS, grads)), dx


def _gru_dir_held(x, w_ih, w_hh, b_ih, b_hh, reverse, steps_b):
    """One GRU direction over [B, S, I] where utterance b holds h at steps t >= steps_b[b]; rows of held steps are zero."""
    bsz, steps, _ = x.shape
    gi = x @ w_ih.t() + b_ih
    h = x.new_zeros(bsz, 256)
    outs = [None] * steps
    for t in (range(steps - 1, -1, -1) if reverse else range(steps)):
        gh = h @ w_hh.t() + b_hh
        i_r, i_z, i_n = gi[:, t].chunk(3, dim=1)
        h_r, h_z, h_n = gh.chunk(3, dim=1)
        r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
        n = torch.tanh(i_n + r * h_n)
        live = (t < steps_b)[:, None]
        h = torch.where(live, (1.0 - z) * n + z * h, h)
        outs[t] = torch.where(live, h, torch.zeros_like(h))
    return torch.stack(outs, dim=1)


def masked_dense(sd, x, frames, labels, dropout_mask=None):
    """The masked dense form in float64 -> (loss, logits, {parameter: gradient}, dx), the layout of ``per_clip_reference``."""
    bsz, t = x.shape[0], x.shape[-1]
    params, full = _leaves(sd)
    fr = torch.as_tensor(list(frames))
    x64 = x.detach().cpu().double().view(bsz, 64, t).clone().requires_grad_(True)
    col = lambda n: torch.arange(n)[None, None, None, :]
    a = torch.where(col(t) < fr[:, None, None, None], x64[:, None], torch.zeros((), dtype=torch.float64))      # 1.
    width = fr
    for i in (1, 2, 3):
        a = F.conv2d(a, full[f"conv{i}.weight"], None, 1, 1)
        inv = torch.rsqrt(full[f"bn{i}.running_var"] + model_ref.BN_EPS) * full[f"bn{i}.weight"]
        a = (a - full[f"bn{i}.running_mean"][None, :, None, None]) * inv[None, :, None, None] + full[f"bn{i}.bias"][None, :, None, None]
        a = F.max_pool2d(torch.relu(a), 2)
        width = width // 2
        a = torch.where(col(a.shape[-1]) < width[:, None, None, None], a, torch.zeros((), dtype=torch.float64))    # 2.
    b_, c, h, w = a.shape
    seq = a.permute(0, 3, 1, 2).contiguous().view(b_, w, c * h)
    for layer in (0, 1):                                                                                           # 3.
        outs = [_gru_dir_held(seq, full[f"gru.weight_ih_l{layer}{s}"], full[f"gru.weight_hh_l{layer}{s}"],
                              full[f"gru.bias_ih_l{layer}{s}"], full[f"gru.bias_hh_l{layer}{s}"], s != "", width) for s in ("", "_reverse")]
        seq = torch.cat(outs, dim=2)
        if layer == 0 and dropout_mask is not None:
            seq = seq * _d(dropout_mask)
    scores = seq @ full["attention.weight"].t() + full["attention.bias"]
    dead = (torch.arange(w)[None, :] >= width[:, None])[:, :, None]
    attn = torch.softmax(scores.masked_fill(dead, float("-inf")), dim=1)                                            # 4.
    ctx = (seq * attn).sum(dim=1)
    logits = ctx @ full["fc.weight"].t() + full["fc.bias"]
    loss = F.cross_entropy(logits, labels)
    grads = torch.autograd.grad(loss, [params[k] for k in model_ref.PARAM_KEYS] + [x64])
    return loss.detach(), logits.detach(), dict(zip(model_ref.PARAM_KEYS, grads)), grads[-1]


def ratio(a, ref):
    """max |a - ref| / rms(ref): the figure the gradient bound is on."""
    ref = ref.detach().cpu().double().flatten()
    return (a.detach().cpu().double().flatten() - ref).abs().max().item() / (ref.pow(2).mean().sqrt().item() + 1e-300)


def grad_ratios(grads, ref_grads):
    """{name: ratio} over the gradients the rule keeps (reference maximum above SKIP_BELOW)."""
    return {k: ratio(grads[k], r) for k, r in ref_grads.items() if r.abs().max().item() > SKIP_BELOW}


# ---- device side (imported lazily: the host tests need no GPU) ----------------------------------------------------------------
def frozen_model(sd, dropout, ncls=31):
    """The module as ``finetune.freeze(model, {"bn_stats"})`` leaves it: train(), bn1..bn3 in eval()."""
    from sir_amd import finetune
    from sir_amd.models.models import CNNAudioGRU
    m = CNNAudioGRU(ncls)
    m.load_state_dict(sd)
    m = m.to("cuda").train()
    finetune.freeze(m, {"bn_stats"})
    m.train()
    m.gru.dropout = dropout
    return m


def ragged_step(m, x, frames, labels, fill=None):
    """One ragged differentiable step on the device -> dict(loss, logits, grads{name}, dx), CPU tensors.  ``fill``: a byte the
    training workspace is filled with before the forward (0xFF: every float a NaN)."""
    from sir_amd import _native, train_ops
    from sir_amd.featurizer import get_featurizer
    xd = x.to("cuda").detach().clone().requires_grad_(True)
    fd = frames if torch.is_tensor(frames) else torch.tensor(list(frames), dtype=torch.int32)
    for p in m.parameters():
        p.grad = None
    if fill is not None:
        st = train_ops._train_state(m)
        need = _native.lib().sir_model_workspace_bytes(get_featurizer().handle, x.shape[0], x.shape[-1], 1)
        st["ws"].get(need, xd.device).fill_(fill)
    logits = m(xd, lengths=fd)                           # (a host tensor is validated on the host, a device tensor by the kernels)
    loss = train_ops.fused_cross_entropy(logits, labels.to("cuda"))
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach().cpu(), "logits": logits.detach().cpu(), "dx": xd.grad.detach().cpu().clone(),
            "grads": {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}}


def device_dropout_mask(m, bsz, t, p):
    """The scaled keep mask [B, S, 512] of the step ``m`` just ran: rebuilt on the host from the step's key (tests/host_rng.py: the
    dense step's hash and element index) and checked bit for bit against workspace slots 8 / 9 (y0d = keep ? y0 / (1 - p) : 0; rows
    t >= S_b are zero in both), the method of test_train_gpu.py::test_dropout_on_training_step_vs_oracle."""
    import host_rng
    import input_grad_ref
    seed, p_used = m._sir_last_dropout
    assert p_used == p
    offs = input_grad_ref.workspace_offsets(bsz, t)
    ws, s = m._sir_train["ws"].buf, t // 8
    n = bsz * s * 512
    keep = torch.from_numpy(host_rng.dropout_keep(seed, n, p)).view(bsz, s, 512)
    y0 = ws[offs[8]: offs[8] + 4 * n].view(torch.float32).view(bsz, s, 512).cpu()
    y0d = ws[offs[9]: offs[9] + 4 * n].view(torch.float32).view(bsz, s, 512).cpu()
    assert torch.equal(y0d, torch.where(keep, y0 * (1.0 / (1.0 - p)), torch.zeros_like(y0)))
    return keep.float() / (1.0 - p)


def zero_tails(x, frames):
    x = x.clone()
    for b, f in enumerate(frames):
        x[b, ..., f:] = 0.0
    return x


def reference_for(m, sd, x, frames, labels, p):
    """``per_clip_reference`` at the device's forward values of the step ``m`` just ran."""
    import input_grad_ref
    bsz, t = x.shape[0], x.shape[-1]
    zo, yo = input_grad_ref.device_forward_values(m, sd, zero_tails(x, frames), bsz, t)
    mask = device_dropout_mask(m, bsz, t, p) if p > 0 else None
    return per_clip_reference(sd, x, frames, labels, zo, yo, mask)


def check_against(out, ref, frames, tag):
    """The parity assertions of one step; prints the measured figures first."""
    ref_loss, ref_logits, ref_grads, ref_dx = ref
    r = grad_ratios(out["grads"], ref_grads)
    r["dx"] = ratio(out["dx"].view(ref_dx.shape), ref_dx)
    lg = (out["logits"].double() - ref_logits).abs().max().item()
    ls = abs(out["loss"].item() - ref_loss.item())
    worst = max(r, key=r.get)
    print(f"{tag}: logits {lg:.2e} loss {ls:.2e} worst gradient {worst} {r[worst]:.2e} dx {r['dx']:.2e}")
    print(f"{tag}: ratios", {k: f"{v:.1e}" for k, v in r.items()})
    assert len(r) >= 29, sorted(r)                       # 28 of the 29 parameters (attention.bias skipped) + dx
    assert lg <= LOGIT_BOUND and ls <= LOSS_BOUND, (lg, ls)
    for k, v in r.items():
        assert v <= GRAD_BOUND, (k, v)
    dx = out["dx"].view(ref_dx.shape)
    for b, f in enumerate(frames):
        assert torch.equal(dx[b, :, f:], torch.zeros_like(dx[b, :, f:])), b
