"""``FusedAdam``: torch.optim.Adam semantics (coupled L2 ``weight_decay``, bias correction, no
AMSGrad -- what the reference builds at scripts/train.py:246-250) with the update of ALL parameter
tensors done by one ``sir_adam_step`` launch (multi-tensor HIP kernel).  State lives in two flat
fp32 buffers (exp_avg, exp_avg_sq) per parameter group.

``max_grad_norm`` folds ``torch.nn.utils.clip_grad_norm_`` over ALL the optimizer's gradients into the step: one extra
read of the gradients (``sir_grad_norm``, per-chunk sums of squares) and ``sir_adam_step_clipped``, which forms the
clip coefficient on the device and updates with ``g * coef``; the ``.grad`` tensors are left unscaled and
``last_grad_norm`` holds ``{total_norm, coef}`` of the last step as a device tensor."""
import ctypes as C

import torch

from . import _native, ops
from .featurizer import get_featurizer


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None):
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError("max_grad_norm must be > 0")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _group_state(self, group):
        gs = self.state.setdefault("_sir_group_%d" % id(group), {})
        if "step" not in gs:
            ps = group["params"]
            n = sum(p.numel() for p in ps)
            gs["step"] = 0
            gs["exp_avg"] = torch.zeros(n, dtype=torch.float32, device=ps[0].device)
            gs["exp_avg_sq"] = torch.zeros(n, dtype=torch.float32, device=ps[0].device)
            offs, off = [], 0
            for p in ps:
                offs.append(off)
                off += p.numel()
            gs["offsets"] = offs
        return gs

    def _norm_partials(self, lib, h):
        """Launch 1 of ``sir_grad_norm`` over every gradient of every group (32 tensors per call, one slab): the Adam
        launches then all form the same global norm from it."""
        from . import train_ops
        grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                 for group in self.param_groups for p in group["params"] if p.grad is not None]
        if not grads:
            return None, 0
        calls, total = [], 0
        for start in range(0, len(grads), 32):
            G, N = train_ops._grad_arrays(grads[start:start + 32])
            calls.append((len(N), G, N, total))
            total += lib.sir_grad_norm_partials(len(N), N)
        part = train_ops.norm_partials(total, grads[0].device)
        for n, G, N, off in calls:
            rc = lib.sir_grad_norm(h, n, G, N, self.max_grad_norm, part.data_ptr() + 4 * off, total - off, None, 0,
                                   _native.current_stream_ptr())
            _native.check(rc, "sir_grad_norm")
        if self.last_grad_norm is None or self.last_grad_norm.device != grads[0].device:
            self.last_grad_norm = torch.empty(2, dtype=torch.float32, device=grads[0].device)
        return part, total

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _native.lib()
        h = get_featurizer().handle
        part, n_part = self._norm_partials(lib, h) if self.max_grad_norm is not None else (None, 0)
        for group in self.param_groups:
            gs = self._group_state(group)
            gs["step"] += 1
            items = [(p, o) for p, o in zip(group["params"], gs["offsets"]) if p.grad is not None]
            for start in range(0, len(items), 32):
                chunk = items[start:start + 32]
                n = len(chunk)
                P, G, M, V = ((C.c_void_p * n)() for _ in range(4))
                N = (C.c_int64 * n)()
                keep = []
                for i, (p, o) in enumerate(chunk):
                    if p.dtype != torch.float32 or not p.is_contiguous():
                        raise _native.SirError("FusedAdam needs contiguous float32 parameters")
                    _native.require_hip(p)
                    g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                    keep.append(g)
                    P[i], G[i] = p.data_ptr(), g.data_ptr()
                    M[i] = gs["exp_avg"].data_ptr() + 4 * o
                    V[i] = gs["exp_avg_sq"].data_ptr() + 4 * o
                    N[i] = p.numel()
                if part is not None:
                    rc = lib.sir_adam_step_clipped(h, n, P, G, M, V, N, gs["step"], float(group["lr"]), float(group["betas"][0]),
                                                   float(group["betas"][1]), float(group["eps"]), float(group["weight_decay"]),
                                                   part.data_ptr(), n_part, self.max_grad_norm, self.last_grad_norm.data_ptr(),
                                                   _native.current_stream_ptr())
                    _native.check(rc, "sir_adam_step_clipped")
                    continue
                rc = lib.sir_adam_step(h, n, P, G, M, V, N, gs["step"], float(group["lr"]), float(group["betas"][0]),
                                       float(group["betas"][1]), float(group["eps"]), float(group["weight_decay"]),
                                       _native.current_stream_ptr())
                _native.check(rc, "sir_adam_step")
        ops.bump_weights_epoch()
        return loss
