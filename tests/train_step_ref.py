"""Shared pieces of the training-step parity tests (``test_train_gpu.py``, ``test_large_batch_gpu.py``,
``test_long_sequence_gpu.py``, ``test_token_range_gpu.py``, ``test_class_count_gpu.py``): views of the step's workspace slots, the values the device's ReLU / max-pool compared (reproduced
bit for bit on the host), the float64 oracle differentiated at those values, and the per-tensor gradient error.  Moved here
unchanged from ``test_train_gpu.py``, whose module docstring gives the method and the bounds.  ``_training_case`` is the whole
check of one step at a batch size and a frame count, moved here from ``test_large_batch_gpu.py``."""
import ctypes as C
import time

import numpy as np
import torch

import cases
import host_rng
import input_grad_ref
from oracle import model_ref
from sir_amd import _native, ops, synth, train_ops
from sir_amd.featurizer import get_featurizer
from sir_amd.models.models import CNNAudioGRU

DEV = "cuda"

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


def _training_case(sd, bsz, t, dropout=0.0, want_dx=False, compare_f32=True, norm_atol=None, oracle_time=False, num_classes=31,
                   labels=None, out=None):
    """One training step of ``bsz`` clips of ``t`` frames against the float64 oracle differentiated at the device's own z / y
    values: loss 2e-5, logits 5e-5, all 29 gradients and the five intermediate gradients of the workspace (divided by the loss
    scale) max |a - b| <= 2e-3 * rms, norms within 1e-3, BN running statistics rtol 1e-4, the input gradient (``want_dx``)
    within ``input_grad_ref.GRAD_BOUND``; with ``dropout`` the keep mask is rebuilt on the host and must equal what the dropout
    kernel wrote.  Prints the float32 oracle's own distance from the float64 one (``compare_f32``) and the device's figures
    before it asserts.  (``test_large_batch_gpu.py``'s, with the frame count as a parameter.)  ``norm_atol`` {parameter name:
    absolute term of that tensor's norm bound in place of 1e-7} is for a gradient that is zero in exact arithmetic, where the
    float32 oracle's own rounding noise exceeds 1e-7 at a shape (the caller's docstring gives both figures); the device's, the
    float32 oracle's and the float64 oracle's values of such a tensor are printed.  ``oracle_time`` prints the CPU seconds of the
    host reproduction of z / y and of the float64 oracle.  ``num_classes`` is the head's size (``sd`` must hold such a head);
    ``labels`` [bsz] replaces the drawn ``synth.synth_labels(bsz, num_classes, ...)``.  Returns the model, its 29 gradients in
    place, for what a caller asserts on top (``test_token_range_gpu.py``: exact zeros); ``out`` (a dict) receives the float64
    oracle's gradients (``ref_grads``) and the printed figures (``test_class_count_gpu.py``: the classifier's gradient row by
    row)."""
    T, S = t, t // 8
    x = cases.varied_features(bsz, T, seed=3000 + bsz)
    y = synth.synth_labels(bsz, num_classes, seed=3001 + bsz) if labels is None else labels
    m = CNNAudioGRU(num_classes)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.gru.dropout = dropout
    m.zero_grad(set_to_none=True)
    xd = x.to(DEV).requires_grad_(want_dx)
    logits = m(xd)
    loss = train_ops.fused_cross_entropy(logits, y.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    mask = None
    if dropout:
        seed, p_used = m._sir_last_dropout
        assert p_used == dropout
        keep = torch.from_numpy(host_rng.dropout_keep(seed, bsz * S * 512, dropout)).view(bsz, S, 512)
        assert 0.45 < keep.float().mean().item() < 0.55
        offs = (C.c_size_t * 40)()
        _native.lib().sir_model_train_workspace_offsets(get_featurizer().handle, bsz, T, offs, 40)
        ws, n = m._sir_train["ws"].buf, bsz * S * 512
        y0 = ws[offs[8]: offs[8] + 4 * n].view(torch.float32).view(bsz, S, 512).cpu()
        y0d = ws[offs[9]: offs[9] + 4 * n].view(torch.float32).view(bsz, S, 512).cpu()
        assert torch.equal(y0d, torch.where(keep, y0 * (1.0 / (1.0 - dropout)), torch.zeros_like(y0)))
        mask = keep.float() / (1.0 - dropout)
    t0 = time.perf_counter()
    v = _views(m, bsz, T)
    zo, yo = _device_forward_values(m, sd, x, bsz, T, v)
    t1 = time.perf_counter()
    st = {}
    ref_loss, ref_grads, ref_stats, ref_logits = _oracle_f64(sd, x, y, zo, yo, dropout_mask=mask, stages=st)
    if oracle_time:
        print(f"B={bsz} T={T}: host z / y {t1 - t0:.1f} s, float64 oracle {time.perf_counter() - t1:.1f} s on {torch.get_num_threads()} threads")
    # the float32 oracle's own distance from the float64 one at the same forward values (printed, not asserted)
    if compare_f32:
        _, g32, _, _ = model_ref.loss_and_grads(sd, x, y, dropout_mask=mask, z_override=zo, y_override=yo)
        own = {k: _rel(g32[k], ref_grads[k])[0] for k in g32 if ref_grads[k].abs().max() > 1e-7}
        own_norm = max(abs(g32[k].double().norm().item() / ref_grads[k].norm().item() - 1.0) for k in own)
        worst = max(own, key=own.get)
        print(f"B={bsz} dropout={dropout}: float32 oracle vs float64 oracle: worst gradient {own[worst]:.1e} * rms ({worst}), worst norm {own_norm:.1e}")
    for name in norm_atol or {}:
        dev = dict(m.named_parameters())[name].grad.double().norm().item()
        f32 = f"{g32[name].double().norm().item():.3e}" if compare_f32 else "not computed"
        print(f"B={bsz}: |{name} gradient|: device {dev:.3e}, float32 oracle {f32}, float64 oracle {ref_grads[name].norm().item():.3e}")
    lerr = abs(loss.item() - ref_loss.item())
    gerr_logits = (logits.detach().cpu().double() - ref_logits).abs().max().item()
    nhwc = lambda a: a.permute(0, 2, 3, 1)
    stages = {"dy1": st["d_gru_l1"], "dy0": st["d_gru_l0"], "dx0": st["d_gru_in"], "da2": nhwc(st["d_conv2"]), "da1": nhwc(st["d_conv1"])}
    serr = {k: _rel(v[k] / _loss_scale(bsz), r)[0] for k, r in stages.items()}
    gerr = _grad_errors(m, ref_grads)
    nerr = {n: abs(p.grad.double().norm().item() - ref_grads[n].norm().item()) / (ref_grads[n].norm().item() + 1e-30)
            for n, p in m.named_parameters() if ref_grads[n].abs().max() > 1e-7}
    print(f"B={bsz}: loss err {lerr:.1e}, logits err {gerr_logits:.1e}, worst gradient {max(gerr.values()):.1e} * rms "
          f"({max(gerr, key=gerr.get)}), worst norm {max(nerr.values()):.1e}, stage gradients / 2^{int(_loss_scale(bsz)).bit_length() - 1}:",
          {k: f"{e:.1e}" for k, e in serr.items()})
    assert lerr < 2e-5
    assert gerr_logits < 5e-5
    for k, e in serr.items():
        assert e < 2e-3, (k, e)
    assert len(gerr) == 29
    for k, e in gerr.items():
        assert e < 2e-3, (k, e)
    for name, p in m.named_parameters():
        rn = ref_grads[name].double().norm().item()
        assert abs(p.grad.double().norm().item() - rn) <= 1e-3 * rn + (norm_atol or {}).get(name, 1e-7), name
    for i in (1, 2, 3):
        bn = getattr(m, f"bn{i}")
        assert torch.allclose(bn.running_mean.cpu().double(), ref_stats[f"bn{i}.running_mean"], rtol=1e-4, atol=1e-6)
        assert torch.allclose(bn.running_var.cpu().double(), ref_stats[f"bn{i}.running_var"], rtol=1e-4, atol=1e-6)
    if want_dx:
        _, _, ref_dx = input_grad_ref.reference(sd, x, zo, yo, labels=y, dropout_mask=mask)
        r = input_grad_ref.ratio(xd.grad, ref_dx)
        print(f"B={bsz}: max|dfeats - ref| / rms(ref) = {r:.2e}")
        assert xd.grad.shape == xd.shape
        assert r <= input_grad_ref.GRAD_BOUND
    if out is not None:
        out.update(ref_grads=ref_grads, loss=lerr, logits=gerr_logits, grad=max(gerr.values()), norm=max(nerr.values()),
                   stage=max(serr.values()), dx=r if want_dx else None)
    ops.check_status()
    return m
