"""Training-step glue: ``torch.autograd`` nodes around the HIP training kernels.

``forward_train(model, x)`` returns logits whose backward runs ``sir_model_train_bwd_emb`` (the one backward
entry point this node calls; the older ones remain for C callers) and hands autograd the 29
parameter gradients as views of ONE flat fp32 buffer (3 261 184 elements); with
``WORLD_SIZE > 1`` that buffer is averaged over ranks with a single RCCL all-reduce before the
views are returned, so the update equals single-GPU training on the global batch.
If ``x.requires_grad`` the backward also returns ``d loss / d x`` (a non-NULL ``dfeats``: the
data chain runs down through conv1); it is rank-local and is not exchanged.
``forward_train_embed`` also returns the 512-float utterance embedding with a graph attached: a loss on it
(``prototypes.ProxyHead``) enters the backward beside ``dlogits`` (a non-NULL ``demb``).
Any number of nodes per module may be live: each holds a training workspace of its own from its forward to the end of its
backward (``sir_amd.leases``), nodes that overlapped return clones instead of the shared views, and a backward whose workspace
has been reused, or whose ``x`` or parameters were changed since its forward, raises ``RuntimeError``.
``fused_cross_entropy`` is the HIP form of the reference's ``nn.CrossEntropyLoss()`` (train.py:242).
Only pointers move through Python; no arithmetic of the step is done by torch ops.
"""
import ctypes as C
import os
from typing import NamedTuple

import torch
from torch.autograd.function import once_differentiable

from . import _native, leases, ops
from .dist_utils import (ShardSampler, all_reduce_mean_, all_reduce_sum_, broadcast_module_,  # noqa: F401
                         init_distributed, limit_host_threads, shutdown_distributed, world_size)
from .featurizer import get_featurizer
from .pipeline import HostStager


class _StepCounter:
    """The process-wide dropout step counter: ``next()`` hands out 1, 2, ... as ``itertools.count(1)`` did; ``value`` (the
    number the NEXT training forward will draw) can be read and set, which is what lets a resumed run continue the mask
    sequence instead of drawing the masks of steps 1, 2, ... again (``sir_amd.run_state``)."""

    def __init__(self):
        self.value = 1

    def __next__(self):
        v = self.value
        self.value = v + 1
        return v


_seed_counter = _StepCounter()


def dropout_step():
    """The counter value the next training forward of this process draws its dropout key from (1 in a new process)."""
    return _seed_counter.value


def set_dropout_step(value):
    value = int(value)
    if value < 1:
        raise ValueError("the dropout step counter starts at 1")
    _seed_counter.value = value


OVERLAP_GRAD_EXCHANGE = os.environ.get("SIR_DDP_OVERLAP", "1") != "0"
HAND_OVER_GRADS = os.environ.get("SIR_HAND_OVER_GRADS", "1") != "0"
# take the data-parallel exchange path even in a ONE-rank process group (bench.py's `rccl_world1` leg and the nccl tests
# on a one-GPU box: the collectives, their stream ordering against the backward kernels and the final scale all run;
# the sum over one rank is the identity)
FORCE_EXCHANGE = os.environ.get("SIR_DDP_FORCE", "0") == "1"


def dropout_seed(step_counter, rank=None):
    """64-bit key of one step's inter-layer dropout mask: the process-local step counter and the data-parallel rank
    (every rank must draw a DIFFERENT mask for its shard, as independent ``nn.GRU`` replicas would)."""
    if rank is None:
        rank = torch.distributed.get_rank() if world_size() > 1 else 0
    return (step_counter * 0x9E3779B97F4A7C15 + rank * 0xD1B54A32D192ED03) % (1 << 64)


def _has_grad_hooks(p):
    return bool(getattr(p, "_backward_hooks", None)) or bool(getattr(p, "_post_accumulate_grad_hooks", None))


def param_list(mod):
    """Parameters in ``named_parameters`` order (== the reference's state_dict order minus buffers)."""
    return [p for _, p in mod.named_parameters()]


# parameter name -> (field of sir_model_grads, index in it or None for a scalar field)
GRAD_FIELDS = {"attention.weight": ("attn_w", None), "attention.bias": ("attn_b", None), "fc.weight": ("fc_w", None), "fc.bias": ("fc_b", None)}
for _i in range(3):
    GRAD_FIELDS.update({f"conv{_i + 1}.weight": ("conv_w", _i), f"bn{_i + 1}.weight": ("bn_w", _i), f"bn{_i + 1}.bias": ("bn_b", _i)})
for _i, _suf in enumerate(ops.GRU_SUFFIXES):
    GRAD_FIELDS.update({"gru.weight_ih" + _suf: ("gru_w_ih", _i), "gru.weight_hh" + _suf: ("gru_w_hh", _i),
                        "gru.bias_ih" + _suf: ("gru_b_ih", _i), "gru.bias_hh" + _suf: ("gru_b_hh", _i)})


class GradBuffer:
    """One flat gradient buffer with per-parameter views + the matching ``sir_model_grads`` struct."""

    def __init__(self, mod):
        params = param_list(mod)
        dev = params[0].device
        self.flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=dev)
        self.views, off = [], 0
        for p in params:
            self.views.append(self.flat[off: off + p.numel()].view_as(p))
            off += p.numel()
        # (named_parameters order: conv1.weight, bn1.weight, bn1.bias, conv2.weight, ... -- looked up by name, not by position)
        self.names = names = [n for n, _ in mod.named_parameters()]
        self.struct = self._fill(_native.ModelGrads(), [True] * len(names))
        self._pruned = {}
        # the conv / BatchNorm gradients come first in named_parameters order; everything behind them (GRU, attention, fc)
        # is final after the first half of the backward
        self.n_cnn = sum(p.numel() for n, p in mod.named_parameters() if n.startswith(("conv", "bn")))
        first_other = next(i for i, n in enumerate(names) if not n.startswith(("conv", "bn")))
        assert all(n.startswith(("conv", "bn")) for n in names[:first_other]) and \
            not any(n.startswith(("conv", "bn")) for n in names[first_other:]), "parameter order changed"

    def _fill(self, g, need):
        """Writes the gradient view of every wanted parameter into its ``sir_model_grads`` field, NULL for the others."""
        for name, v, n in zip(self.names, self.views, need):
            field, i = GRAD_FIELDS[name]
            ptr = v.data_ptr() if n else None
            if i is None:
                setattr(g, field, ptr)
            else:
                getattr(g, field)[i] = ptr
        return g

    def struct_for(self, need):
        """``sir_model_grads`` with NULL for every parameter whose gradient is not wanted (``need``: one bool per
        parameter, ``named_parameters`` order): the backward then skips what only feeds those.  Returns the struct and
        whether any conv / BatchNorm gradient is wanted."""
        hit = self._pruned.get(need)                 # (keyed by autograd's own tuple: nothing is rebuilt per step)
        if hit is not None:
            return hit
        key, need = need, tuple(bool(n) for n in need)
        if all(need):
            g = self.struct
        else:
            g = self._fill(_native.ModelGrads(), need)
        cnn = any(n for name, n in zip(self.names, need) if name.startswith(("conv", "bn")))
        self._pruned[key] = (g, cnn)
        return g, cnn


def bn_config(mod):
    """``sir_train_config`` of the next step: ``bnK.training == False`` freezes that block's statistics, as in torch."""
    key = (mod.bn1.training, mod.bn2.training, mod.bn3.training)
    cfg = _configs.get(key)
    if cfg is None:
        cfg = _configs[key] = _native.TrainConfig()
        for i in range(3):
            cfg.bn_frozen[i] = 0 if key[i] else 1
    return cfg


_configs = {}


def step_config(mod):
    """(``sir_train_config``, dropout p) of the next step from the sub-modules' own flags, as torch reads them
    (``gru.training == False`` turns the inter-layer dropout off)."""
    return bn_config(mod), (float(mod.gru.dropout) if mod.gru.training else 0.0)


_freeze_checked = set()


def _check_same_freeze(need, cfg, device="cuda"):
    """Data parallel: every rank must freeze the same set (the collectives are sized by it).  Checked once per set with
    the MAX-reduce pattern of ``ops.check_status``: a 64-bit digest and its complement agree on all ranks only if equal."""
    import torch.distributed as dist
    key = (tuple(bool(n) for n in need), tuple(cfg.bn_frozen))
    if key in _freeze_checked:
        return
    bits = sum(1 << i for i, b in enumerate(key[0] + tuple(bool(f) for f in key[1])) if b)
    t = torch.tensor([bits, -bits], dtype=torch.int64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    hi, neg_lo = (int(v) for v in t.tolist())
    if hi != bits or -neg_lo != bits:
        raise _native.SirError("the ranks of this job froze different parameter / BatchNorm sets: every rank must call "
                               "finetune.freeze with the same arguments")
    _freeze_checked.add(key)


def _train_state(mod):
    """The module's gradient buffer, its training workspace and the pool that leases it (and spares) to the nodes.  The
    buffer's views are cut for one set of parameters: it is rebuilt whenever the model took a new token since
    (``ops.cached_weights`` -- call it first -- hands one out when a parameter or sub-module was replaced, e.g. a new head
    with another class count), never written through stale views."""
    st = getattr(mod, "_sir_train", None)
    token = getattr(mod, "_sir_token", None)
    if st is None or st["token"] != token or st["grads"].flat.device != next(mod.parameters()).device:
        ws = st["ws"] if st is not None else ops.Workspace()
        pool = st.get("pool") if st is not None else None
        st = {"grads": GradBuffer(mod), "ws": ws, "pool": pool or leases.LeasePool(ws, ops.Workspace), "token": token}
        mod._sir_train = st
    return st


def _input_stamp(mod):
    """What a node's backward must find as its forward left it: torch's in-place version counter of every parameter and the
    count of parameter writes behind those counters (``ops._params_epoch``: ``FusedAdam.step``, ``weights_changed``,
    ``broadcast_module_``).  A training forward's own running-statistics update is not counted: a live block's backward uses
    the batch statistics its forward left in the workspace, a frozen block's the folded scale / shift there, so a second
    node's forward is no stale input of the first."""
    return ops._params_epoch[0], tuple(map(ops._tensor_version, param_list(mod)))


def _bn_ptr_arrays(mod):
    rm = (C.c_void_p * 3)(*[getattr(mod, f"bn{i}").running_mean.data_ptr() for i in (1, 2, 3)])
    rv = (C.c_void_p * 3)(*[getattr(mod, f"bn{i}").running_var.data_ptr() for i in (1, 2, 3)])
    return rm, rv


def _scratch_running_stats(mod, st, cfg, rm, rv):
    """Crafting pass: point the running-statistics update of every LIVE BatchNorm block at a scratch buffer kept beside the
    module's training state (the kernels only write it for such a block: its forward and backward use the batch statistics),
    so that ``running_mean`` / ``running_var`` stay as they are bit for bit.  Frozen blocks keep the module's pointers: they
    are read, never written."""
    dev = next(mod.parameters()).device
    scratch = st.get("craft_bn")
    if scratch is None or scratch[0].device != dev:
        scratch = st["craft_bn"] = [torch.zeros(2, getattr(mod, f"bn{i}").num_features, dtype=torch.float32, device=dev)
                                    for i in (1, 2, 3)]
    for i in range(3):
        if not cfg.bn_frozen[i]:
            rm[i], rv[i] = scratch[i][0].data_ptr(), scratch[i][1].data_ptr()


class StepOptions(NamedTuple):
    """The settings of one ``_TrainStep``.  ``step == False`` (sir_amd.explain) draws no dropout key and leaves the step counter
    and ``mod._sir_last_dropout`` alone; ``craft == True`` (``forward_craft``) also keeps the LIVE BatchNorm blocks' running
    statistics, ``num_batches_tracked`` and the cached-weights epoch as they are.  ``frames`` (device int32 ``[B]``): the ragged
    step, ``sir_model_train_fwd_ragged`` and a non-NULL ``frames`` of the backward.  ``want_emb`` (``forward_train_embed``): the
    node returns ``(logits, emb)``."""
    cfg: _native.TrainConfig
    dropout_p: float
    step: bool = True
    craft: bool = False
    frames: torch.Tensor = None
    want_emb: bool = False


def _run_forward(lib, h, w, rm, rv, x, momentum, seed, opts, logits, ws):
    """The step's native forward: ``sir_model_train_fwd_ragged`` when ``opts.frames`` is given (frozen statistics: it takes no
    momentum), else ``sir_model_train_fwd_cfg``."""
    bsz, _, t = x.shape
    head = (h, C.byref(w), rm, rv, x.data_ptr())
    tail = (float(opts.dropout_p), seed, C.byref(opts.cfg), logits.data_ptr(), ws.data_ptr(), ws.numel(), _native.current_stream_ptr())
    if opts.frames is not None:
        rc, who = lib.sir_model_train_fwd_ragged(*head, opts.frames.data_ptr(), bsz, t, *tail), "sir_model_train_fwd_ragged"
    else:
        rc, who = lib.sir_model_train_fwd_cfg(*head, bsz, t, momentum, *tail), "sir_model_train_fwd_cfg"
    _native.check(rc, who)


class _TrainStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mod, opts, *params):
        cfg, dropout_p, craft, frames = opts.cfg, opts.dropout_p, opts.craft, opts.frames
        lib = _native.lib()
        h = get_featurizer().handle
        x_shape = x.shape
        x = ops._as_features(x)
        bsz, _, t = x.shape
        w, keep = ops.cached_weights(mod)
        st = _train_state(mod)
        need = lib.sir_model_workspace_bytes(h, bsz, t, 1)
        if need == 0:
            raise _native.SirError(f"unsupported shape batch={bsz} frames={t} ({ops.SHAPE_LIMITS})")
        # a workspace no live node holds: the module's own unless an earlier node has still to run its backward.  ctx is the
        # lease's only owner, so a node that is dropped without a backward gives the workspace back when it is collected.
        ctx.lease = lease = st["pool"].take()
        ws = lease.slot.get(need, x.device)
        rm, rv = _bn_ptr_arrays(mod)
        if craft:
            _scratch_running_stats(mod, st, cfg, rm, rv)
        logits = torch.empty((bsz, w.num_classes), dtype=torch.float32, device=x.device)
        seed = 0
        if opts.step:
            seed = dropout_seed(next(_seed_counter))
            mod._sir_last_dropout = (seed, float(dropout_p))  # lets tests rebuild the mask (tests/dropout_host.py)
        momentum = float(mod.bn1.momentum if mod.bn1.momentum is not None else 0.1)
        _run_forward(lib, h, w, rm, rv, x, momentum, seed, opts, logits, ws)
        live = [] if craft else [getattr(mod, f"bn{i + 1}").num_batches_tracked for i in range(3) if not cfg.bn_frozen[i]]
        if live:                                     # frozen statistics: nothing was written, cached layouts stay valid
            ops.bump_weights_epoch(parameters=False) # BN running statistics were updated in place
            torch._foreach_add_(live, 1)
        # x through torch's own version check (an in-place change before the backward raises there); the parameters and the
        # writes torch does not count through the stamp
        ctx.save_for_backward(x)
        ctx.stamp = _input_stamp(mod)
        ctx.mod, ctx.seed, ctx.dropout_p, ctx.ws, ctx.cfg = mod, seed, float(dropout_p), ws, cfg
        ctx.x_shape, ctx.frames = x_shape, frames
        if opts.want_emb:
            # the attention-pooled context the forward left in its workspace slot, copied on the stream -- the next step reuses
            # the workspace, a view would dangle.  A gradient that is not there stays None.
            ctx.set_materialize_grads(False)
            at = _train_offsets(h, bsz, t)[CTX_SLOT]
            return logits, ws[at: at + 4 * bsz * 512].view(torch.float32).view(bsz, 512).clone()
        return logits

    @staticmethod
    @once_differentiable
    def backward(ctx, dlogits, demb=None):
        try:
            (x,) = ctx.saved_tensors                 # (raises if x was changed in place since the forward)
            ctx.lease.check()
            if _input_stamp(ctx.mod) != ctx.stamp:
                raise RuntimeError("a parameter of the model was changed in place between this node's forward and its backward "
                                   "(an optimizer step, weights_changed(), a broadcast): the backward would differentiate the "
                                   "saved activations against the new weights -- run the forward again")
            return _TrainStep._backward(ctx, x, dlogits, demb)
        finally:
            # the end of the node's backward, not the collection of its graph, frees the workspace: in the ordinary loop the
            # previous loss is still alive when the next forward runs
            ctx.lease.release()

    @staticmethod
    def _backward(ctx, x, dlogits, demb):
        lib = _native.lib()
        mod = ctx.mod
        h = get_featurizer().handle
        w, keep = ops.cached_weights(mod)
        st = _train_state(mod)
        bsz, _, t = x.shape
        if dlogits is None:                          # (the two-output node with no loss on the logits: dlogits stays required)
            if demb is None:
                return (None, None, None) + (None,) * len(param_list(mod))
            dlogits = torch.zeros((bsz, w.num_classes), dtype=torch.float32, device=x.device)
        dlogits = dlogits.contiguous()
        if demb is not None:
            demb = demb.to(torch.float32).contiguous()
        grads = st["grads"]
        params = param_list(mod)
        need = ctx.needs_input_grad[3:]
        # d loss / d x, returned in the caller's shape ([B,64,T] and [B,1,64,T] are the same memory); None: not wanted
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None

        def ptr(v):
            return v.data_ptr() if v is not None else None

        def run(part):
            # the one backward of this node (include/sir_hip.h): a NULL frames is the padded step, a NULL demb lets no gradient
            # in at the embedding, a NULL dfeats writes no input gradient -- same launches and bits as the entry points without them
            rc = lib.sir_model_train_bwd_emb(h, C.byref(w), x.data_ptr(), ptr(ctx.frames), dlogits.data_ptr(), ptr(demb), bsz, t,
                                             ctx.dropout_p, ctx.seed, C.byref(ctx.cfg), C.byref(gstruct), ptr(dx), ctx.ws.data_ptr(),
                                             ctx.ws.numel(), part, _native.current_stream_ptr())
            _native.check(rc, "sir_model_train_bwd_emb")

        if not any(need):
            # only the input gradient is wanted: no parameter gradient is written, so nothing is exchanged between ranks
            # and no .grad is touched
            gstruct, _ = grads.struct_for(need)
            run(_native.BWD_ALL)
            return (dx.view(ctx.x_shape), None, None) + (None,) * len(params)
        # a .grad left over from the previous step that still aliases the flat buffer (no zero_grad in between:
        # gradient accumulation) must be detached from it before the kernels overwrite the buffer
        for p, v in zip(params, grads.views):
            if p.grad is not None and p.grad.data_ptr() == v.data_ptr():
                p.grad = p.grad.clone()

        gstruct, cnn = grads.struct_for(need)        # only the trainable views: NULL = not wanted, not computed
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            _check_same_freeze(need, ctx.cfg)

        _exchange_and_scale(grads, run, cnn=cnn, dx=dx is not None)
        dx = dx.view(ctx.x_shape) if dx is not None else None
        if ctx.lease.shared:
            # another node of this module is or was live beside this one: its kernels write the same flat buffer, and autograd
            # holds what is returned here by reference until both have run -- tensors of this node's own
            return (dx, None, None) + tuple(v.clone() if n else None for v, n in zip(grads.views, need))
        if HAND_OVER_GRADS and all(p.grad is None and not _has_grad_hooks(p) for p in params):
            # zero_grad(set_to_none=True) (train.py:90): the views of the flat buffer BECOME the .grad tensors; returning
            # them through autograd would make AccumulateGrad clone all 29 of them (29 copy launches per step)
            for p, v, n in zip(params, grads.views, need):
                if n:
                    p.grad = v
            return (dx, None, None) + (None,) * len(params)
        return (dx, None, None) + tuple(v if n else None for v, n in zip(grads.views, need))


_offsets = {}
CTX_SLOT = 11        # the training workspace's slot of the attention-pooled context, fp32 [B, 512]: the embedding


def _train_offsets(h, bsz, t):
    """Byte offsets of the training workspace's slots (``sir_model_train_workspace_offsets``), kept per shape."""
    offs = _offsets.get((bsz, t))
    if offs is None:
        buf = (C.c_size_t * 48)()
        if _native.lib().sir_model_train_workspace_offsets(h, bsz, t, buf, 48) <= CTX_SLOT:
            raise _native.SirError("sir_model_train_workspace_offsets failed")
        offs = _offsets[(bsz, t)] = list(buf)
    return offs


def _exchange_and_scale(grads, run, cnn=True, dx=False):
    """The per-step gradient exchange around the two halves of the backward (``run(part)`` launches one half, or
    nothing for a rank that has no batch).  ``cnn=False`` (every conv / BatchNorm parameter frozen): the second half and
    its bucket are left out -- on every rank alike, ``zero_contribution_step`` included.  ``dx=True`` (the gradient of
    the input features is wanted): the second half runs even then -- it writes that gradient, which stays on its rank --
    but its bucket is still left out."""
    import torch.distributed as dist
    world = world_size()
    forced = FORCE_EXCHANGE and dist.is_available() and dist.is_initialized()
    if (world > 1 or forced) and OVERLAP_GRAD_EXCHANGE:
        # data parallel: the GRU / attention / fc gradients (96 % of the 13 MB) are final after the first half of the
        # backward; their all-reduce runs beside the conv backward, the small conv / BN bucket follows
        run(_native.BWD_HEAD_GRU)
        tail = grads.flat[grads.n_cnn:]
        work = dist.all_reduce(tail, op=dist.ReduceOp.SUM, async_op=True)
        if cnn or dx:
            run(_native.BWD_CNN)
        if cnn:
            dist.all_reduce(grads.flat[:grads.n_cnn], op=dist.ReduceOp.SUM)
        work.wait()
        (grads.flat if cnn else tail).mul_(1.0 / world)
    else:
        run(_native.BWD_ALL)
        bucket = grads.flat if cnn else grads.flat[grads.n_cnn:]     # (a frozen CNN's region was not written: not exchanged)
        if forced:                              # un-overlapped form of the same exchange
            dist.all_reduce(bucket, op=dist.ReduceOp.SUM)
            bucket.mul_(1.0 / world)
        else:
            all_reduce_mean_(bucket)            # the one exchange step of data-parallel training


def zero_contribution_step(mod):
    """Data-parallel step of a rank whose batch is empty (``collate_fn`` dropped every item, train.py:67-68 / :82-83):
    the other ranks are inside the gradient all-reduce, so this rank joins the same collectives with a zero gradient
    and ends up with the same averaged ``.grad`` as they do (the caller then runs ``optimizer.step()`` like everyone
    else, keeping the replicas identical).  Without it the job would hang on the mismatched collective."""
    st = _train_state(mod)
    grads = st["grads"]
    params = param_list(mod)
    for p, v in zip(params, grads.views):
        if p.grad is not None and p.grad.data_ptr() == v.data_ptr():
            p.grad = None
    grads.flat.zero_()
    _exchange_and_scale(grads, lambda part: None,
                        cnn=any(p.requires_grad for n, p in mod.named_parameters() if n.startswith(("conv", "bn"))))
    for p, v in zip(params, grads.views):
        if p.requires_grad:
            p.grad = v


def ragged_frames(lengths, x):
    """``lengths`` of a ragged differentiable call as the device int32 ``[B]`` the kernels take: ``ops._as_lengths`` after the
    shape checks on ``x`` -- a host list or CPU tensor is validated here, before any launch; a device tensor goes through the
    status word (bad rows come back NaN, ``ops.check_status`` raises)."""
    xf = ops._as_features(x)
    return ops._as_lengths(lengths, xf.shape[0], xf.shape[2], x.device)


def forward_train(mod, x, lengths=None):
    """Training-mode forward of ``CNNAudioGRU`` (batch-statistics BN, inter-layer dropout
    ``mod.gru.dropout``), differentiable wrt the module's parameters and, if ``x.requires_grad``, wrt ``x`` (``x.grad`` has
    the shape of ``x``; a double backward raises).  The sub-modules' own flags are honoured as torch
    honours them: ``bnK.eval()`` freezes that block's statistics (forward and backward), ``gru.eval()`` turns the dropout
    off, and a parameter with ``requires_grad == False`` gets no gradient -- the backward stops where the trainable
    parameters stop (a NULL gradient pointer of ``sir_model_train_bwd_emb``, the one backward the node calls).

    ``lengths`` (int tensor or list, frames per clip): the un-padded function and its gradient -- row b is what the model gives
    ``x[b:b+1, ..., :lengths[b]]`` on its own (``sir_model_train_fwd_ragged`` / ``frames`` of the backward).  It needs bn1, bn2 and
    bn3 in ``eval()``, which is what ``finetune.freeze(model, {"bn_stats"})`` leaves; otherwise ``SirError``."""
    return _forward_step(mod, x, lengths, want_emb=False)


def forward_train_embed(mod, x, lengths=None):
    """``forward_train`` with a second output: ``(logits, emb)``, ``emb`` float32 ``[B, 512]`` the attention-pooled context that
    ``model.embed`` returns in eval, here with the graph attached.  A loss may be put on either or both: the backward hands
    ``(dlogits, demb)`` to ``sir_model_train_bwd_emb``, which adds ``demb`` to the ``dctx`` it forms from ``dlogits`` (zeros when
    only the embedding carries a loss) -- same freeze / pruning rules, flat gradient buffer and data-parallel exchange as
    ``forward_train``.  With no gradient on ``emb`` the step is ``forward_train``'s, bit for bit."""
    return _forward_step(mod, x, lengths, want_emb=True)


def _forward_step(mod, x, lengths, want_emb):
    cfg, dropout_p = step_config(mod)
    if lengths is not None and not all(cfg.bn_frozen):
        raise _native.SirError("lengths (un-padded clips) on the differentiable path need bn1, bn2 and bn3 on their running statistics: "
                               "freeze them first (finetune.freeze(model, {'bn_stats'}) or bnK.eval()), call model.eval(), or run "
                               "under torch.no_grad() -- with live batch statistics a clip has no result of its own")
    _native.require_hip(x)
    ops._as_features(x)                              # (shape / dtype checks; the node itself takes x in the caller's shape)
    frames = ragged_frames(lengths, x) if lengths is not None else None
    return _TrainStep.apply(x, mod, StepOptions(cfg, dropout_p, frames=frames, want_emb=want_emb), *param_list(mod))


def forward_craft(mod, x):
    """``(logits, leaf)`` of the crafting pass of an adversary: the training-path forward with the module's own flags
    (``bnK.eval()`` blocks on their running statistics, the others on batch statistics) and NO side effect -- inter-layer
    dropout off and no key drawn (``dropout_step()`` unchanged), running statistics, ``num_batches_tracked`` and the
    cached-weights epoch untouched.  ``leaf`` is ``x`` detached with ``requires_grad``; ``torch.autograd.grad(loss, leaf)`` runs
    the backward with all 29 gradient pointers NULL: no ``p.grad`` is touched and nothing is exchanged between
    ranks."""
    _native.require_hip(x)
    ops._as_features(x)
    leaf = x.detach().requires_grad_(True)
    opts = StepOptions(cfg=bn_config(mod), dropout_p=0.0, step=False, craft=True)
    with torch.enable_grad():
        logits = _TrainStep.apply(leaf, mod, opts, *[p.detach() for p in param_list(mod)])
    return logits, leaf


class MetricLoss:
    """The ``metric_loss`` of ``train()``: a ``prototypes.ProxyHead`` on the embedding beside the classifier's loss.  It rides on
    the model like an ``Adversary`` (``set_metric_loss``), so ``train_epoch`` / ``train_epoch_waveforms`` keep the reference's
    signatures.  ``loss(model, x, label, loss_fn)`` is the step's loss, ``ce_weight * loss_fn(logits, label) + weight *
    head(emb, label)``, from one ``forward_with_embedding``; ``sync_grad()`` averages the proxies' gradient over the ranks (the
    model's own gradients are exchanged inside the backward), ``zero_contribution()`` is an empty shard's part in that."""

    def __init__(self, head, weight=1.0, ce_weight=1.0):
        weight, ce_weight = float(weight), float(ce_weight)
        if not weight >= 0.0 or not ce_weight >= 0.0:
            raise ValueError("metric_loss: weight and ce_weight must be >= 0")
        self.head, self.weight, self.ce_weight = head, weight, ce_weight

    def loss(self, model, x, label, loss_fn):
        logits, emb = model.forward_with_embedding(x)
        return self.ce_weight * loss_fn(logits, label) + self.weight * self.head(emb, label)

    def sync_grad(self):
        if world_size() > 1 and self.head.proxies.grad is not None:
            all_reduce_mean_(self.head.proxies.grad)

    def zero_contribution(self):
        self.head.proxies.grad = torch.zeros_like(self.head.proxies)
        self.sync_grad()


def set_metric_loss(mod, metric):
    """Make ``train_epoch`` / ``train_epoch_waveforms`` add ``metric`` (a ``MetricLoss``; ``None``: stop) to the step's loss.
    Nothing else reads it: ``validate`` and ``predict`` are unaffected and it is not part of ``state_dict()``."""
    if metric is not None and not isinstance(metric, MetricLoss):
        raise TypeError("set_metric_loss takes a train_ops.MetricLoss or None")
    mod._sir_metric_loss = metric
    return metric


def metric_loss_of(mod):
    return getattr(mod, "_sir_metric_loss", None)


def _adv_check(eps, alpha, *tensors):
    """Host-side validation of ``adv_step``: raises before any device call."""
    eps, alpha = float(eps), float(alpha)
    if not eps >= 0.0:
        raise ValueError("eps must be >= 0")
    if not alpha >= 0.0:
        raise ValueError("alpha must be >= 0")
    shape = None
    for name, v in tensors:
        if v is None:
            continue
        sh = ops.check_feature_batch(v, name, 1)
        if sh[0] < 1:
            raise ValueError(f"{name}: expected at least one clip, got {tuple(v.shape)}")
        if shape is not None and sh != shape:
            raise ValueError(f"{name}: shape {tuple(v.shape)} does not match x0's batch {shape[0]} and {shape[1]} frames")
        shape = sh
    if any(v is not None and not v.is_cuda for _, v in tensors):
        raise _native.SirError("tensor is not on a HIP device: this path runs on MI355X only (no CPU fallback)")
    return eps, alpha, shape


def adv_step(x0, x, g, eps, alpha, active=None, seed=0, keep_zero_columns=True, out=None):
    """One ascent / projection step of an L-infinity adversary by ``sir_adv_step`` (include/sir_hip.h has the arithmetic).
    ``g`` given: ``clamp(x + alpha * sign(g), x0 - eps, x0 + eps)``; ``x`` and ``g`` both ``None``: the random start
    ``x0 + eps * (2 U - 1)`` keyed by ``seed``.  Rows with ``active[b] == 0`` (device int32 ``[B]``; ``None`` = all active) and,
    with ``keep_zero_columns``, all-zero frame columns of ``x0`` come back as bit-exact copies of ``x0``.  float32 HIP tensors
    ``[B,64,T]`` or ``[B,1,64,T]`` only; ``out`` may be ``x`` (in place), never ``x0`` or ``g``.  Returns ``out`` (a new tensor
    in the shape of ``x0`` when not given).  Every argument is validated before any device call."""
    if g is None and x is not None:
        raise ValueError("x given without g: a random start is drawn around x0 alone")
    if g is not None and x is None:
        raise ValueError("a gradient step needs the iterate x (pass x0 for the first step)")
    eps, alpha, (bsz, t) = _adv_check(eps, alpha, ("x0", x0), ("x", x), ("g", g), ("out", out))
    if active is not None:
        if not torch.is_tensor(active) or active.dtype != torch.int32 or active.dim() != 1 or active.numel() != bsz:
            raise ValueError("active must be an int32 tensor with one flag per row")
        if not active.is_cuda:
            raise _native.SirError("tensor is not on a HIP device: this path runs on MI355X only (no CPU fallback)")
    for name, v in (("x0", x0), ("x", x), ("g", g), ("out", out)):
        if v is not None and not v.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if out is not None and (out is x0 or out is g):
        raise ValueError("out must not be x0 or g (it may be x)")
    seed = int(seed)
    if not 0 <= seed < (1 << 64):
        raise ValueError("seed must fit 64 bits")
    if out is None:
        out = torch.empty_like(x0)
    cfg = _native.AdvConfig(eps, alpha, 1 if keep_zero_columns else 0)
    rc = _native.lib().sir_adv_step(get_featurizer().handle, x0.data_ptr(), x.data_ptr() if x is not None else None,
                                    g.data_ptr() if g is not None else None,
                                    active.contiguous().data_ptr() if active is not None else None, bsz, 64, t, C.byref(cfg), seed,
                                    out.data_ptr(), _native.current_stream_ptr())
    _native.check(rc, "sir_adv_step")
    return out


def default_adv_alpha(eps, steps, random_start):
    """The step size of an ``Adversary`` that was given none: ``eps`` for one step from ``x`` itself (FGSM), ``1.25 eps`` for one
    step from a random start (Wong et al. 2020), ``2.5 eps / steps`` otherwise (Madry et al. 2018)."""
    if steps == 1:
        return 1.25 * eps if random_start else eps
    return 2.5 * eps / steps


def set_adversary(mod, adversary):
    """Make ``train_epoch`` / ``train_epoch_waveforms`` craft adversarial examples for ``mod`` with ``adversary`` (``None``: stop).
    The adversary rides on the model as the LR scheduler rides on the optimizer (``step_scheduler_with``): both epoch functions
    keep the reference's signatures.  Nothing else reads it -- ``validate``, ``predict`` and ``sir_amd.explain`` are unaffected,
    and it is not part of ``state_dict()`` (its generator travels in the run state, ``sir_amd.run_state``)."""
    if adversary is not None and not isinstance(adversary, Adversary):
        raise TypeError("set_adversary takes a train_ops.Adversary or None")
    mod._sir_adversary = adversary
    return adversary


def adversary_of(mod):
    return getattr(mod, "_sir_adversary", None)


class Adversary:
    """L-infinity adversarial training (FGSM / PGD) for ``train_epoch`` / ``train_epoch_waveforms`` (``set_adversary``), modelled on ``Mixup``: the
    host ``random.Random(seed)`` in ``.rng`` draws, per batch, the ``active`` flags (each row with probability ``prob``: clean
    and adversarial rows share one batch and one BatchNorm pass) and one 64-bit ``start_seed``.  ``draw(bsz)`` returns them as
    ``(int32 [B] host tensor, int)``; both are drawn for every batch whatever the settings, so the sequence depends on the
    seed and the batch sizes alone.  The flags are staged through pinned buffers (no device sync); the seed travels by value.

    ``adversary(model, x, loss_closure)`` returns the detached ``x_adv`` in the shape of ``x`` after ``steps`` crafting passes
    (``forward_craft``: the module is left as it was found); ``loss_closure(logits)`` is the loss to ascend -- the step's own
    training loss.  All-zero frame columns of ``x`` (padding, SpecAugment time bands) are kept.  ``eps == 0`` still runs the
    passes and returns the bits of ``x`` (for an ``x`` without -0.0)."""

    def __init__(self, eps, alpha=None, steps=1, random_start=True, prob=1.0, seed=0):
        import random
        eps, steps, prob = float(eps), int(steps), float(prob)
        if not eps >= 0.0:
            raise ValueError("adversarial eps must be >= 0")
        if steps < 1:
            raise ValueError("adversarial steps must be >= 1")
        if not 0.0 <= prob <= 1.0:
            raise ValueError("adversarial prob must be in [0, 1]")
        self.eps, self.steps, self.prob, self.random_start = eps, steps, prob, bool(random_start)
        self.alpha = default_adv_alpha(eps, steps, self.random_start) if alpha is None else float(alpha)
        if not self.alpha >= 0.0:
            raise ValueError("adversarial alpha must be >= 0")
        self.rng = random.Random(int(seed))
        self._stage = None

    def draw(self, bsz):
        flags = [1 if self.rng.random() < self.prob else 0 for _ in range(bsz)]
        return torch.tensor(flags, dtype=torch.int32), self.rng.getrandbits(64)

    def __call__(self, model, x, loss_closure):
        _adv_check(self.eps, self.alpha, ("x", x))
        if self._stage is None or self._stage.device != x.device:
            self._stage = HostStager(x.device)
        flags, start_seed = self.draw(x.shape[0])
        active = self._stage(flags)
        x0 = x.detach().contiguous()
        cur = x0
        if self.random_start:
            cur = adv_step(x0, None, None, self.eps, self.alpha, active, seed=start_seed)
        for _ in range(self.steps):
            logits, leaf = forward_craft(model, cur)
            with torch.enable_grad():
                loss = loss_closure(logits)
            (g,) = torch.autograd.grad(loss, leaf)
            cur = adv_step(x0, cur, g, self.eps, self.alpha, active, out=None if cur is x0 else cur)
        return cur


class _FusedCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, labels_b=None, lam=None, label_smoothing=0.0):
        lib = _native.lib()
        logits = logits.contiguous()
        labels = labels.to(torch.int64).contiguous()
        _native.require_hip(logits, labels)
        bsz, ncls = logits.shape
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        dlogits = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        h, dptr = get_featurizer().handle, dlogits.data_ptr() if dlogits is not None else None
        if labels_b is None and lam is None and label_smoothing == 0.0:
            rc = lib.sir_ce_loss(h, logits.data_ptr(), labels.data_ptr(), bsz, ncls, loss.data_ptr(), dptr, 1.0,
                                 _native.current_stream_ptr())
            _native.check(rc, "sir_ce_loss")
        else:
            if lam is not None and labels_b is None:
                raise _native.SirError("fused_cross_entropy: lam weighs labels against labels_b, which was not given")
            if labels_b is not None:
                labels_b = labels_b.to(torch.int64).contiguous()
                if labels_b.shape != labels.shape:
                    raise _native.SirError("fused_cross_entropy: labels_b must have the shape of labels")
            if lam is not None:
                lam = lam.to(torch.float32).contiguous()
                if lam.numel() != bsz:
                    raise _native.SirError("fused_cross_entropy: lam must hold one value per row")
            _native.require_hip(labels_b, lam)
            rc = lib.sir_ce_loss_soft(h, logits.data_ptr(), labels.data_ptr(),
                                      labels_b.data_ptr() if labels_b is not None else None,
                                      lam.data_ptr() if lam is not None else None, float(label_smoothing), bsz, ncls,
                                      loss.data_ptr(), dptr, 1.0, _native.current_stream_ptr())
            _native.check(rc, "sir_ce_loss_soft")
        ctx.dlogits = dlogits
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        # loss.backward() passes 1.0; a general scalar is applied by the (tiny) multiply below
        return ctx.dlogits * grad_out, None, None, None, None


def fused_cross_entropy(logits, labels, labels_b=None, lam=None, label_smoothing=0.0):
    """``nn.CrossEntropyLoss()`` (mean over the batch) computed by ``sir_ce_loss``.  With any of the three optional
    arguments, ``sir_ce_loss_soft``: the target of row b is ``(1 - eps) * (lam[b] * e[labels[b]] + (1 - lam[b]) *
    e[labels_b[b]]) + eps / C`` -- ``nn.CrossEntropyLoss(label_smoothing=eps)``, and mixup's two-label loss
    ``lam * CE(l, ya) + (1 - lam) * CE(l, yb)`` with a per-row ``lam`` (device float32 ``[B]``; ``None`` = all 1)."""
    return _FusedCE.apply(logits, labels, labels_b, lam, label_smoothing)


def mix_features(x, perm, lam):
    """``lam[:, None, None] * x + (1 - lam[:, None, None]) * x[perm]`` for a feature batch ``[B, 64, T]`` (``T % 4 == 0``)
    by ``sir_mix_features``: out of place, fp32 ``fma(lam, a, (1 - lam) * b)``; a row with ``lam == 1`` is a bit-exact
    copy.  ``perm`` int64 ``[B]`` and ``lam`` float32 ``[B]`` are device tensors; an entry of ``perm`` outside ``[0, B)``
    gives a zero row and ``SirError`` at the next ``ops.check_status()``."""
    _native.require_hip(x, perm, lam)
    x = ops._as_features(x)
    bsz, n_mels, t = x.shape
    perm = perm.to(torch.int64).contiguous()
    lam = lam.to(torch.float32).contiguous()
    if perm.numel() != bsz or lam.numel() != bsz:
        raise _native.SirError("mix_features: perm and lam must hold one value per row")
    out = torch.empty_like(x)
    rc = _native.lib().sir_mix_features(get_featurizer().handle, x.data_ptr(), perm.data_ptr(), lam.data_ptr(), bsz, n_mels, t,
                                        out.data_ptr(), _native.current_stream_ptr())
    _native.check(rc, "sir_mix_features")
    return out


class Mixup:
    """mixup (Zhang et al. 2018) for ``train_epoch`` / ``train_epoch_waveforms``: per batch ONE ``lam ~ Beta(alpha, alpha)``
    and one permutation of the rows, drawn on the host (``random.Random(seed)``: same seed, same sequence; no device
    call).  ``draw(bsz)`` returns the host tensors ``(perm int64 [B], lam float32 [B])``; calling the object with a device
    batch stages them through pinned buffers, mixes the features with ``mix_features`` and returns
    ``(mixed, labels[perm], lam)`` -- the arguments ``fused_cross_entropy`` takes after ``labels``."""

    def __init__(self, alpha, seed=0):
        import random
        if not alpha > 0:
            raise ValueError("mixup alpha must be > 0")
        self.alpha = float(alpha)
        self.rng = random.Random(int(seed))
        self._stage = None

    def draw(self, bsz):
        lam = self.rng.betavariate(self.alpha, self.alpha)
        perm = list(range(bsz))
        self.rng.shuffle(perm)
        return torch.tensor(perm, dtype=torch.int64), torch.full((bsz,), lam, dtype=torch.float32)

    def __call__(self, x, labels):
        if self._stage is None or self._stage.device != x.device:
            self._stage = HostStager(x.device)
        perm, lam = self.draw(x.shape[0])
        perm, lam = self._stage(perm), self._stage(lam)
        return mix_features(x, perm, lam), labels[perm], lam


_norm_partials = {}


def _grad_arrays(grads):
    n = len(grads)
    G, N = (C.c_void_p * n)(), (C.c_int64 * n)()
    for i, g in enumerate(grads):
        if g.dtype != torch.float32 or not g.is_contiguous():
            raise _native.SirError("gradient clipping needs contiguous float32 gradients")
        _native.require_hip(g)
        G[i], N[i] = g.data_ptr(), g.numel()
    return G, N


def norm_partials(n_floats, device):
    """Grow-only device slab for the per-chunk sums of squares (reused step after step: stream order protects it)."""
    buf = _norm_partials.get(device)
    if buf is None or buf.numel() < n_floats:
        buf = _norm_partials[device] = torch.empty(max(n_floats, 1024), dtype=torch.float32, device=device)
    return buf


def clip_grad_norm_(parameters, max_norm):
    """``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` (2-norm, ``error_if_nonfinite=False``) in two launches of
    ``sir_grad_norm``: the gradients are scaled in place by ``min(1, max_norm / (norm + 1e-6))`` and the total norm comes
    back as a device scalar -- nothing synchronises with the host.  Parameters without a gradient (frozen) are left out;
    the norm is an ordered reduction, bit-reproducible run to run."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.zeros(())
    if len(grads) > 32:
        raise _native.SirError(f"clip_grad_norm_: {len(grads)} gradient tensors, at most 32 per call (the model has 29)")
    lib = _native.lib()
    G, N = _grad_arrays(grads)
    n = lib.sir_grad_norm_partials(len(grads), N)
    part = norm_partials(n, grads[0].device)
    out2 = torch.empty(2, dtype=torch.float32, device=grads[0].device)
    rc = lib.sir_grad_norm(get_featurizer().handle, len(grads), G, N, float(max_norm), part.data_ptr(), part.numel(),
                           out2.data_ptr(), 1, _native.current_stream_ptr())
    _native.check(rc, "sir_grad_norm")
    return out2[0]
