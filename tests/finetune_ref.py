"""Functional statement of one fine-tuning step of ``CNNAudioGRU`` (CPU, fp32 or fp64): the torch idiom

    model.train(); bnK.eval() for the frozen blocks; requires_grad_(False) on the frozen parameters

written out over a plain ``state_dict``.  A frozen block normalises with ``running_mean`` / ``running_var`` (eps 1e-5) as
constants -- so its backward is the affine form dz = dy * gamma * invstd_running with no mean terms -- and leaves them alone; a
live block uses the batch statistics and returns its updated running statistics (momentum 0.1, unbiased variance).  PINNED to the
reference's own module by ``tests/golden/finetune_golden.npz`` (``test_finetune_host.py``); the GRU, attention and head are the
oracle's (``oracle/model_ref.py``, itself pinned by ``model_golden.npz``).

ReLU and max-pool are not differentiable at ties: two correct fp32 forwards can route a gradient to different pixels.  As the
B = 256 tests of ``test_train_gpu.py`` do, ``z_override`` / ``y_override`` {block: [B,C,H,W]} substitute the VALUES the device's
ReLU / pooling compared (conv output and BatchNorm output) straight-through, so that the reference differentiates at the device's
decisions while every gradient still flows through this file's own arithmetic.
"""
import torch
import torch.nn.functional as F

from oracle import model_ref

BN_EPS = 1e-5
BN_MOMENTUM = 0.1
PARAM_KEYS = tuple(model_ref.PARAM_KEYS)


def batchnorm(z, sd, i, frozen, new_stats):
    """BatchNorm2d of block ``i`` on z [B,C,H,W]: running statistics as constants when ``frozen``, else batch statistics."""
    gamma, beta = sd[f"bn{i}.weight"], sd[f"bn{i}.bias"]
    if frozen:
        mean, var = sd[f"bn{i}.running_mean"].detach(), sd[f"bn{i}.running_var"].detach()
    else:
        mean = z.mean(dim=(0, 2, 3))
        var = z.var(dim=(0, 2, 3), unbiased=False)
        n = z.numel() // z.shape[1]
        new_stats[f"bn{i}.running_mean"] = ((1 - BN_MOMENTUM) * sd[f"bn{i}.running_mean"] + BN_MOMENTUM * mean).detach()
        new_stats[f"bn{i}.running_var"] = ((1 - BN_MOMENTUM) * sd[f"bn{i}.running_var"] + BN_MOMENTUM * var * (n / (n - 1))).detach()
    xhat = (z - mean[None, :, None, None]) * torch.rsqrt(var + BN_EPS)[None, :, None, None]
    return xhat * gamma[None, :, None, None] + beta[None, :, None, None]


def forward(sd, x, bn_frozen=(False, False, False), new_stats=None, dropout_mask=None, z_override=None, y_override=None):
    """x [B,64,T] or [B,1,64,T] -> logits; ``bn_frozen[k]`` is ``not bn{k+1}.training``."""
    if new_stats is None:
        new_stats = {}
    if x.dim() == 3:
        x = x.unsqueeze(1)
    for i in (1, 2, 3):
        x = F.conv2d(x, sd[f"conv{i}.weight"], bias=None, stride=1, padding=1)
        if z_override is not None and i in z_override:
            x = x + (z_override[i] - x).detach()
        x = batchnorm(x, sd, i, bool(bn_frozen[i - 1]), new_stats)
        if y_override is not None and i in y_override:
            x = x + (y_override[i] - x).detach()
        x = F.max_pool2d(torch.relu(x), 2)
    b, c, h, w = x.shape
    seq = x.permute(0, 3, 1, 2).contiguous().view(b, w, c * h)
    y = model_ref.bigru(seq, sd, dropout_mask)
    attn = torch.softmax(y @ sd["attention.weight"].t() + sd["attention.bias"], dim=1)
    return (y * attn).sum(dim=1) @ sd["fc.weight"].t() + sd["fc.bias"]


def loss_and_grads(sd, x, labels, bn_frozen=(False, False, False), trainable=None, dropout_mask=None, z_override=None,
                   y_override=None):
    """One step: CE (mean) loss, {name: gradient} for the names in ``trainable`` (default: all 29), the running statistics
    after the step (every block; a frozen block's are the inputs, untouched) and the logits."""
    names = [k for k in PARAM_KEYS if trainable is None or k in trainable]
    params = {k: sd[k].detach().clone().requires_grad_(True) for k in names}
    full = {k: v.detach() for k, v in sd.items()}
    full.update(params)
    new_stats = {}
    logits = forward(full, x, bn_frozen, new_stats, dropout_mask, z_override, y_override)
    loss = F.cross_entropy(logits, labels)
    grads = torch.autograd.grad(loss, [params[k] for k in names])
    stats = {}
    for i in (1, 2, 3):
        for s in ("running_mean", "running_var"):
            stats[f"bn{i}.{s}"] = new_stats.get(f"bn{i}.{s}", sd[f"bn{i}.{s}"].detach())
    return loss.detach(), dict(zip(names, grads)), stats, logits.detach()
