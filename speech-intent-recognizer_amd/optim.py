"""``FusedAdam``: torch.optim.Adam semantics (coupled L2 ``weight_decay``, bias correction, no
AMSGrad -- what the reference builds at scripts/train.py:246-250) with the update of ALL parameter
tensors done by one ``sir_adam_step`` launch (multi-tensor HIP kernel).  State lives in two flat
fp32 buffers (exp_avg, exp_avg_sq) per parameter group.

``max_grad_norm`` folds ``torch.nn.utils.clip_grad_norm_`` over ALL the optimizer's gradients into the step: one extra
read of the gradients (``sir_grad_norm``, per-chunk sums of squares) and ``sir_adam_step_clipped``, which forms the
clip coefficient on the device and updates with ``g * coef``; the ``.grad`` tensors are left unscaled and
``last_grad_norm`` holds ``{total_norm, coef}`` of the last step as a device tensor.

``decoupled_weight_decay=True`` gives ``torch.optim.AdamW`` and ``ema_decay=d`` keeps an exponential moving average of the
stepped parameters (the "shadow": a third flat buffer per group, a copy of the parameters before the first update,
``shadow = d * shadow + (1 - d) * p_new`` inside the same launch); either one routes the step through ``sir_adam_step_ex``.
With neither, ``step()`` issues the launches it always issued.

The state is keyed by the group's INDEX (``"_sir_group_0"``, ...), so that ``state_dict()`` / ``load_state_dict()`` carry
the step count, both moments and the shadow into a fresh process; a state whose flat sizes differ from the groups' raises."""
import contextlib
import ctypes as C

import torch

from . import _native, ops
from .featurizer import get_featurizer


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 decoupled_weight_decay=False, ema_decay=None, ema_warmup=False):
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError("max_grad_norm must be > 0")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        if ema_decay is not None and not 0.0 < ema_decay < 1.0:
            raise ValueError("ema_decay must lie in (0, 1)")
        self.decoupled_weight_decay = bool(decoupled_weight_decay)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @staticmethod
    def _key(index):
        return "_sir_group_%d" % index

    def _group_state(self, index):
        group = self.param_groups[index]
        gs = self.state.setdefault(self._key(index), {})
        if "step" not in gs:
            ps = group["params"]
            n = sum(p.numel() for p in ps)
            gs["step"] = 0
            gs["exp_avg"] = torch.zeros(n, dtype=torch.float32, device=ps[0].device)
            gs["exp_avg_sq"] = torch.zeros(n, dtype=torch.float32, device=ps[0].device)
        if "offsets" not in gs:                       # (derived from the group: not part of a saved state)
            offs, off = [], 0
            for p in group["params"]:
                offs.append(off)
                off += p.numel()
            gs["offsets"] = offs
        if self.ema_decay is not None and "ema" not in gs:
            with torch.no_grad():                     # the shadow starts as a copy of the parameters
                gs["ema"] = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in group["params"]])
        return gs

    # ---- the EMA shadow --------------------------------------------------------------------------------------------
    def ema_decay_at(self, step):
        """The decay of 1-based step ``step``: ``ema_decay``, or ``min(ema_decay, (1 + t) / (10 + t))`` with ``ema_warmup``."""
        if self.ema_decay is None:
            raise ValueError("this optimizer keeps no EMA (ema_decay=None)")
        return min(self.ema_decay, (1.0 + step) / (10.0 + step)) if self.ema_warmup else self.ema_decay

    def ema_params(self):
        """``[(parameter, shadow view shaped like it), ...]`` over every parameter the optimizer steps (the shadow is
        created here if no step has run yet: a bit-exact copy of the parameters)."""
        if self.ema_decay is None:
            raise ValueError("this optimizer keeps no EMA (ema_decay=None)")
        out = []
        for index, group in enumerate(self.param_groups):
            gs = self._group_state(index)
            for p, o in zip(group["params"], gs["offsets"]):
                out.append((p, gs["ema"][o:o + p.numel()].view_as(p)))
        return out

    def ema_state_dict(self, model):
        """``model.state_dict()`` (copies) with the shadow in place of every parameter this optimizer steps; frozen
        parameters and the BatchNorm buffers are the live model's."""
        shadow = {id(p): e for p, e in self.ema_params()}
        names = {name: id(p) for name, p in model.named_parameters()}
        out = {}
        for name, t in model.state_dict().items():
            src = shadow.get(names.get(name), t)
            out[name] = src.detach().clone()
        return out

    @contextlib.contextmanager
    def swapped_ema(self):
        """Exchange live and shadow values in place, and back on exit (validation / checkpointing with the averaged
        weights; once per epoch, plain copies).  Inference rebuilds its derived weight layouts both times."""
        def swap():
            with torch.no_grad():
                for p, e in self.ema_params():
                    tmp = p.detach().clone()
                    p.copy_(e)
                    e.copy_(tmp)
            ops.bump_weights_epoch()
        swap()
        try:
            yield self
        finally:
            swap()

    # ---- state that survives the process ---------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        """``torch.optim.Optimizer.load_state_dict`` plus what it cannot know about the flat buffers: they are checked
        against the parameter groups BEFORE anything is taken over (a state that does not fit raises; it never restarts
        the moments from zero) and moved to the parameters' device."""
        state, groups = state_dict["state"], state_dict["param_groups"]
        if len(groups) != len(self.param_groups):
            raise ValueError(f"FusedAdam.load_state_dict: the state has {len(groups)} parameter groups, the optimizer {len(self.param_groups)}")
        fresh = {}
        for index, group in enumerate(self.param_groups):
            want = sum(p.numel() for p in group["params"])
            gs = state.get(self._key(index))
            if gs is None:
                if any(str(k).startswith("_sir_group_") for k in state):
                    raise ValueError(f"FusedAdam.load_state_dict: no state under {self._key(index)!r} (keys {sorted(map(str, state))}): "
                                     "written by a version that keyed the state by a process address; it cannot be resumed")
                continue                              # a state saved before the first step
            have = {k: int(gs[k].numel()) for k in ("exp_avg", "exp_avg_sq", "ema") if k in gs}
            if "exp_avg" not in have or "exp_avg_sq" not in have or any(n != want for n in have.values()):
                raise ValueError(f"FusedAdam.load_state_dict: group {index} holds {want} elements in {len(group['params'])} tensors, "
                                 f"the saved flat buffers hold {have}")
            if ("ema" in have) != (self.ema_decay is not None):
                raise ValueError(f"FusedAdam.load_state_dict: the saved state {'has' if 'ema' in have else 'has no'} EMA shadow, "
                                 f"this optimizer was built with ema_decay={self.ema_decay}")
            dev = group["params"][0].device
            fresh[self._key(index)] = dict(
                {k: gs[k].detach().to(device=dev, dtype=torch.float32, copy=True).contiguous() for k in have}, step=int(gs["step"]))
        super().load_state_dict({"state": {}, "param_groups": groups})
        self.state.update(fresh)

    def state_dict(self):
        """Step count, both moments and the shadow of every group under ``"_sir_group_<index>"`` (the tensors are the live
        buffers, as for every torch optimizer: ``torch.save`` or copy them before the next step)."""
        sd = super().state_dict()
        sd["state"] = {k: {n: v for n, v in gs.items() if n != "offsets"} for k, gs in sd["state"].items()}
        return sd

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
        extended = self.decoupled_weight_decay or self.ema_decay is not None
        for index, group in enumerate(self.param_groups):
            gs = self._group_state(index)
            gs["step"] += 1
            items = [(p, o) for p, o in zip(group["params"], gs["offsets"]) if p.grad is not None]
            for start in range(0, len(items), 32):
                chunk = items[start:start + 32]
                n = len(chunk)
                P, G, M, V = ((C.c_void_p * n)() for _ in range(4))
                E = (C.c_void_p * n)() if self.ema_decay is not None else None
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
                    if E is not None:
                        E[i] = gs["ema"].data_ptr() + 4 * o
                    N[i] = p.numel()
                if extended:                          # a new option is on: the one call that covers every variant
                    cfg = _native.AdamConfig(float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]),
                                             float(group["eps"]), float(group["weight_decay"]), int(self.decoupled_weight_decay),
                                             self.max_grad_norm if part is not None else 0.0,
                                             self.ema_decay_at(gs["step"]) if E is not None else 0.0)
                    rc = lib.sir_adam_step_ex(h, n, P, G, M, V, E, N, gs["step"], C.byref(cfg),
                                              part.data_ptr() if part is not None else None, n_part,
                                              self.last_grad_norm.data_ptr() if part is not None else None,
                                              _native.current_stream_ptr())
                    _native.check(rc, "sir_adam_step_ex")
                    continue
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
