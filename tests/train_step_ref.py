"""Shared pieces of the training-step parity tests (``test_train_gpu.py``, ``test_large_batch_gpu.py``): views of the step's
workspace slots, the values the device's ReLU / max-pool compared (reproduced bit for bit on the host), the float64 oracle
differentiated at those values, and the per-tensor gradient error.  Moved here unchanged from ``test_train_gpu.py``, whose
module docstring gives the method and the bounds."""
import ctypes as C

import numpy as np
import torch

from oracle import model_ref
from sir_amd import _native
from sir_amd.featurizer import get_featurizer

TB = {"a1": 0, "z2": 1, "a2": 2, "z3": 3, "x0": 4, "y0": 8, "y1": 10, "ctx": 11,
      "dy1": 21, "dy0": 22, "dgi": 23, "dgh": 24, "dx0": 25, "dz3": 26, "da2": 27, "dz2": 28, "da1": 29}


def _views(m, bsz, t):
    lib = _native.lib()
    offs = (C.c_size_t * 40)()       # (slot indices: the list at sir_model_train_workspace_offsets in include/sir_hip.h)
    n = lib.sir_model_train_workspace_offsets(get_featurizer().handle, bsz, t, offs, 40)
    assert n > 0
    ws = m._sir_train["ws"].buf
    wp1, wp2 = t // 2, t // 4
    s = wp2 // 2
    shp = {"a1": (bsz, 32, wp1, 32), "z2": (bsz, 32, wp1, 64), "a2": (bsz, 16, wp2, 64), "z3": (bsz, 16, wp2, 128),
           "x0": (bsz, s, 1024), "y0": (bsz, s, 512), "y1": (bsz, s, 512), "ctx": (bsz, 512),
           "dy1": (bsz, s, 512), "dy0": (bsz, s, 512), "dx0": (bsz, s, 1024), "da2": (bsz, 16, wp2, 64),
           "da1": (bsz, 32, wp1, 32), "dz3": (bsz, 16, wp2, 128), "dz2": (bsz, 32, wp1, 64)}
    out = {}
    for k, sh in shp.items():
        numel = int(np.prod(sh))
        out[k] = ws[offs[TB[k]]: offs[TB[k]] + 4 * numel].view(torch.float32).view(sh).cpu()
    return out


def _loss_scale(bsz):
    """The backward's internal loss scale (csrc/train_workspace.h::sir_bwd_loss_scale): 2^8 x batch rounded up to a power of two.  The
    intermediate gradients in the workspace carry it (the parameter gradients do not)."""
    k = 8
    while (1 << (k - 8)) < bsz and k < 24:
        k += 1
    return float(1 << k)


def _rel(a, b):
    a, b = a.detach().cpu().double().flatten(), b.detach().cpu().double().flatten()
    rms = b.pow(2).mean().sqrt().item()
    return (a - b).abs().max().item() / (rms + 1e-30), rms


def _fma32(a, b, c):
    """float32 fma(a, b, c) emulated through float64 (the product of two floats is exact there)."""
    return (a.double() * b.double() + c.double()).float()


def _device_forward_values(m, sd, x, bsz, t, v):
    """What the device's ReLU / max-pool compared, reproduced bit for bit on the host: z (conv outputs) and
    y = fma(z, scale, shift) of the three blocks, NCHW.  z2 / z3 are read from the workspace; z1 (never stored on the
    device) is the same chain of nine fmas per output that conv1's kernels evaluate; scale / shift are the device's."""
    lib = _native.lib()
    offs = (C.c_size_t * 40)()
    lib.sir_model_train_workspace_offsets(get_featurizer().handle, bsz, t, offs, 40)
    bn = m._sir_train["ws"].buf[offs[12]: offs[12] + 4 * 448].view(torch.float32).cpu()
    scale, shift = bn[:224], bn[224:448]
    xp = torch.nn.functional.pad(x.float(), (1, 1, 1, 1))                     # [B, 66, T + 2]
    w1 = sd["conv1.weight"].float().view(32, 9)
    z1 = torch.zeros(bsz, 32, 64, t)
    for ky in range(3):
        for kx in range(3):
            z1 = _fma32(xp[:, None, ky:ky + 64, kx:kx + t], w1[None, :, ky * 3 + kx, None, None], z1)
    nchw = lambda a: a.permute(0, 3, 1, 2)
    z = {1: z1, 2: nchw(v["z2"]), 3: nchw(v["z3"])}
    y = {i: _fma32(z[i], scale[o:o + c][None, :, None, None], shift[o:o + c][None, :, None, None])
         for i, o, c in ((1, 0, 32), (2, 32, 64), (3, 96, 128))}
    return z, y


def _oracle_f64(sd, x, y, zo, yo, dropout_mask=None, stages=None):
    """The oracle's backward in FLOAT64 at the device's forward values (z / y overrides, themselves fp32 device values).  At B = 256 a
    convolution weight gradient is a sum of 3.3 M products that largely cancel: the fp32 CPU backward carries up to ~1e-2 of
    rms in it, and how much depends on how many threads split the sum (seen: 6.6e-4 with the box's default pool, 8.3e-3 once an
    earlier test had capped the pool at the CPU quota) -- the reference for these two tests is therefore computed in double."""
    d = lambda t: t.double() if torch.is_tensor(t) and t.is_floating_point() else t
    sd64 = {k: d(v) for k, v in sd.items()}
    zo64 = {k: d(v) for k, v in zo.items()}
    yo64 = {k: d(v) for k, v in yo.items()}
    loss, grads, stats, logits = model_ref.loss_and_grads(sd64, d(x), y, dropout_mask=d(dropout_mask) if dropout_mask is not None else None,
                                                          stages=stages, z_override=zo64, y_override=yo64)
    return loss, grads, stats, logits


def _grad_errors(m, ref_grads):
    out = {}
    for name, p in m.named_parameters():
        if ref_grads[name].abs().max() <= 1e-7:
            out[name] = float((p.grad.cpu() - ref_grads[name]).abs().max())
        else:
            out[name] = _rel(p.grad, ref_grads[name])[0]
    return out
