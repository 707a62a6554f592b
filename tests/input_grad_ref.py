"""Shared pieces of the input-gradient tests (``test_input_grad_gpu.py``): the float64 reference for ``d out / d x`` and the
device's forward values it is evaluated at.

Reference: ``oracle.model_ref.forward`` in float64 with ``x.requires_grad_()`` and ``torch.autograd.grad``, evaluated at the
values the device's ReLU / max-pool compared (``z_override`` / ``y_override``, the method of
``test_train_gpu.py::test_ragged_training_step_vs_oracle``), so that no pooling or ReLU tie can route a gradient differently
and no element has to be excluded.  ``model_ref.forward`` has ONE ``train`` flag for the three BatchNorms; the one mixed case
(bn1 frozen, bn2 / bn3 live) therefore goes through ``tests/finetune_ref.py::forward``, the same statement with a flag per
block (pinned to the reference's module by ``finetune_golden.npz``).

Bound: the project's gradient bound, ``max |a - b| <= 2e-3 * rms(reference)``.
"""
import ctypes as C

import torch
import torch.nn.functional as F

import finetune_ref
from oracle import model_ref
from sir_amd import _native
from sir_amd.featurizer import get_featurizer

GRAD_BOUND = 2e-3


def _d(v):
    return v.double() if torch.is_tensor(v) and v.is_floating_point() else v


def fma32(a, b, c):
    """float32 fma(a, b, c) through float64 (the product of two floats is exact there)."""
    return (a.double() * b.double() + c.double()).float()


def workspace_offsets(bsz, t):
    offs = (C.c_size_t * 40)()
    assert _native.lib().sir_model_train_workspace_offsets(get_featurizer().handle, bsz, t, offs, 40) > 29
    return offs


def device_forward_values(m, sd, x, bsz, t):
    """z (conv outputs) and y = fma(z, scale, shift) of the three blocks as the device's last training-path forward of ``m``
    saw them, NCHW fp32: z2 / z3 from workspace slots 1 / 3, z1 (never stored) as conv1's chain of nine fmas in tap order,
    scale / shift from slot 12."""
    offs = workspace_offsets(bsz, t)
    ws = m._sir_train["ws"].buf
    wp1, wp2 = t // 2, t // 4
    z2 = ws[offs[1]: offs[1] + 4 * bsz * 32 * wp1 * 64].view(torch.float32).view(bsz, 32, wp1, 64).cpu()
    z3 = ws[offs[3]: offs[3] + 4 * bsz * 16 * wp2 * 128].view(torch.float32).view(bsz, 16, wp2, 128).cpu()
    bn = ws[offs[12]: offs[12] + 4 * 448].view(torch.float32).cpu()
    scale, shift = bn[:224], bn[224:448]
    x = x.detach().cpu().float().view(bsz, 64, t)
    xp = F.pad(x, (1, 1, 1, 1))
    w1 = sd["conv1.weight"].float().view(32, 9)
    z1 = torch.zeros(bsz, 32, 64, t)
    for ky in range(3):
        for kx in range(3):
            z1 = fma32(xp[:, None, ky:ky + 64, kx:kx + t], w1[None, :, ky * 3 + kx, None, None], z1)
    z = {1: z1, 2: z2.permute(0, 3, 1, 2), 3: z3.permute(0, 3, 1, 2)}
    y = {i: fma32(z[i], scale[o:o + c][None, :, None, None], shift[o:o + c][None, :, None, None])
         for i, o, c in ((1, 0, 32), (2, 32, 64), (3, 96, 128))}
    return z, y


def reference(sd, x, zo, yo, labels=None, target=None, bn_frozen=(False, False, False), dropout_mask=None, dlogits=None):
    """float64: ``(out, logits, d out / d x)`` with ``out`` = mean cross-entropy against ``labels``, or the sum over the rows
    of ``logits[b, target[b]]`` (rows are independent when every BatchNorm is frozen, the only use of ``target``), or, with
    ``dlogits`` [B, C], ``(logits * dlogits).sum()``: the vector-Jacobian product the device computes for that upstream gradient."""
    sd64 = {k: _d(v) for k, v in sd.items()}
    zo64, yo64 = {k: _d(v) for k, v in zo.items()}, {k: _d(v) for k, v in yo.items()}
    x64 = x.detach().cpu().double().view(x.shape[0], 64, x.shape[-1]).requires_grad_()
    mask = _d(dropout_mask)
    frozen = tuple(bool(f) for f in bn_frozen)
    if frozen in ((False,) * 3, (True,) * 3):
        logits = model_ref.forward(sd64, x64, train=not frozen[0], dropout_mask=mask, z_override=zo64, y_override=yo64)
    else:
        logits = finetune_ref.forward(sd64, x64, frozen, None, mask, zo64, yo64)
    if dlogits is not None:
        out = (logits * dlogits.detach().cpu().double()).sum()
    else:
        out = F.cross_entropy(logits, labels) if target is None else logits.gather(1, target.view(-1, 1)).sum()
    (dx,) = torch.autograd.grad(out, x64)
    return out.detach(), logits.detach(), dx


def ratio(dx, ref):
    """max |dx - ref| / rms(ref): the figure the bound is on."""
    ref = ref.double().flatten()
    return (dx.detach().cpu().double().flatten() - ref).abs().max().item() / (ref.pow(2).mean().sqrt().item() + 1e-300)


def launch_counts(fn):
    """Runs ``fn`` with every kernel group timed (one-stream form) and returns {profile name: launches}."""
    lib, h = _native.lib(), get_featurizer().handle
    nk = lib.sir_profile_kernel_count() + _native.PROFILE_EXTRA_IDS      # (the new id lies behind the count: include/sir_hip.h)
    names = [lib.sir_profile_kernel_name(i).decode() for i in range(nk)]
    ms, cnt = (C.c_double * nk)(), (C.c_int64 * nk)()
    _native.check(lib.sir_profile_enable(h, 1, -1), "sir_profile_enable")
    try:
        fn()
    finally:
        lib.sir_profile_collect(h, ms, cnt, nk)
        _native.check(lib.sir_profile_enable(h, 0, -1), "sir_profile_enable")
    return {names[i]: int(cnt[i]) for i in range(nk)}, {names[i]: float(ms[i]) for i in range(nk)}
