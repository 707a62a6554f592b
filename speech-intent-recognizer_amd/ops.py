"""Host glue between ``torch`` tensors and the C ABI for the model path.

Only pointer plumbing lives here: tensors stay owned by torch, the HIP library
gets ``data_ptr()``s plus the current stream.  No arithmetic is done in Python
and nothing falls back to ``torch.nn`` compute.
"""
import ctypes as C
import itertools
import operator

import torch

from . import _native
from .featurizer import get_featurizer

GRU_SUFFIXES = ("_l0", "_l0_reverse", "_l1", "_l1_reverse")
WS_NAMES = ("conv1", "conv2", "gru_in", "gi", "gru_l0", "gru_l1", "ctx")
# what every model entry point accepts (csrc/model_shape.h: the GRU runs frames / 8 steps, the attention kernels hold 256)
SHAPE_LIMITS = "need 8 <= frames <= 2055 (at most 256 GRU steps), batch <= 65535"


def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise _native.SirError(f"{name} must be contiguous float32")
    if not t.is_cuda:
        raise _native.SirError(f"{name} is not on a HIP device (no CPU fallback)")
    return t


_WEIGHT_MODULES = ("conv1", "bn1", "conv2", "bn2", "conv3", "bn3", "gru", "attention", "fc")


def _weight_slots(mod):
    """``(sub-modules, slots)``: the nine sub-modules that own weights and, per tensor ``sir_model_weights`` points at,
    ``(the owner's _parameters / _buffers dict, key, reference name)``.  The order is the one ``weights_struct`` fills."""
    try:
        mods = [mod._modules[n] for n in _WEIGHT_MODULES]
    except KeyError as e:
        raise _native.SirError(f"sub-module {e} is missing from the module") from None
    slots = []
    for i in range(3):
        conv, bn = mods[2 * i], mods[2 * i + 1]
        slots.append((conv._parameters, "weight", f"conv{i + 1}.weight"))
        slots.append((bn._parameters, "weight", f"bn{i + 1}.weight"))
        slots.append((bn._parameters, "bias", f"bn{i + 1}.bias"))
        slots.append((bn._buffers, "running_mean", f"bn{i + 1}.running_mean"))
        slots.append((bn._buffers, "running_var", f"bn{i + 1}.running_var"))
    gru = mods[6]._parameters
    for suf in GRU_SUFFIXES:
        for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            slots.append((gru, kind + suf, "gru." + kind + suf))
    for name, m in (("attention", mods[7]), ("fc", mods[8])):
        slots.append((m._parameters, "weight", name + ".weight"))
        slots.append((m._parameters, "bias", name + ".bias"))
    return mods, slots


def weights_struct(mod, slots=None):
    """sir_model_weights filled with the module's parameter/buffer pointers (reference key names)."""
    if slots is None:
        slots = _weight_slots(mod)[1]
    keep = []
    for d, k, name in slots:
        t = d.get(k)
        if t is None:
            raise _native.SirError(f"{name} is missing from the module")
        keep.append(_f32c(t.detach(), name))
    ptrs = iter([t.data_ptr() for t in keep])
    w = _native.ModelWeights()
    for i in range(3):
        w.conv_w[i], w.bn_w[i], w.bn_b[i], w.bn_mean[i], w.bn_var[i] = (next(ptrs) for _ in range(5))
    for i in range(4):
        w.gru_w_ih[i], w.gru_w_hh[i], w.gru_b_ih[i], w.gru_b_hh[i] = (next(ptrs) for _ in range(4))
    w.attn_w, w.attn_b, w.fc_w, w.fc_b = (next(ptrs) for _ in range(4))
    w.num_classes = keep[-2].shape[0]
    return w, keep


def cached_weights(mod):
    """The pointer struct and the tensors it points at, rebuilt when the module no longer holds those tensors.
    ``CNNAudioGRU._apply`` / ``load_state_dict`` drop the cache; every other route that REPLACES a tensor -- a new head
    (``model.fc = nn.Linear(...)``), ``nn.Parameter`` assignment, ``p.data = t``, ``vector_to_parameters``, a child's own
    ``.cpu()`` / ``.to()`` -- is caught here, per call, by comparing the nine sub-modules and the storage addresses the module
    holds NOW with the cached ones; the model then takes a new token, as after ``load_state_dict``.  In-place updates keep
    the pointers valid (``weights_version`` covers those that torch counts, ``CNNAudioGRU.weights_changed`` the rest)."""
    cache = getattr(mod, "_sir_wcache", None)
    if cache is not None:
        try:
            mods, slots = mod._sir_wsrc
            m = mod._modules
            if [m[n] for n in _WEIGHT_MODULES] == mods and \
                    tuple(map(_tensor_address, [d[k] for d, k, _ in slots])) == mod._sir_wptrs:
                return cache
        except (AttributeError, KeyError, TypeError):    # a tensor or sub-module was removed: the rebuild below names it
            pass
        mod._sir_token = new_model_token()
    mods, slots = _weight_slots(mod)
    cache = weights_struct(mod, slots)
    mod._sir_wcache = cache
    mod._sir_wsrc = (mods, slots)
    mod._sir_wptrs = tuple(t.data_ptr() for t in cache[1])
    return cache


_weights_epoch = [1]
_params_epoch = [1]       # the bumps of _weights_epoch that wrote parameters (bump_weights_epoch)
_tensor_version = operator.attrgetter("_version")
_tensor_address = torch.Tensor.data_ptr              # (unbound, mapped at C level: this runs on every model call)
_model_tokens = itertools.count(1)


def new_model_token():
    """Process-unique id of one set of weights: ``CNNAudioGRU`` takes one in ``__init__`` and a fresh one whenever its
    storage or contents are replaced wholesale (``_apply``, ``load_state_dict``, a copy of the module) or ``cached_weights``
    finds a tensor or sub-module replaced.  ``id(module)`` is NOT such an id: a freed module's address is reused by the next
    one built in the same place."""
    return next(_model_tokens)


def bump_weights_epoch(parameters=True):
    """Called by everything that rewrites parameters/buffers behind torch's back (the HIP Adam step, the
    training forward's running-statistics update, ``broadcast_module_``'s writes through ``.data``), so that
    cached derived weight layouts are rebuilt.  ``parameters=False`` (the training forward alone): only BatchNorm running
    statistics were written, which no backward reads -- the parameters epoch, which a live node of the differentiable step
    compares between its forward and its backward (``train_ops._input_stamp``), stays."""
    _weights_epoch[0] += 1
    if parameters:
        _params_epoch[0] += 1


def weights_version(mod, keep, workspace=None):
    """Non-zero 64-bit fingerprint of (the global epoch, the model's token, torch's in-place version counters, the
    storage addresses of every parameter / buffer, the generation of the workspace that holds the prepared layouts).
    Two different models, a moved or reloaded model, or a re-allocated workspace can therefore never present the
    library with the version under which another set of weights was prepared."""
    token = getattr(mod, "_sir_token", None)
    if token is None:
        token = mod._sir_token = new_model_token()
    ptrs = getattr(mod, "_sir_wptrs", None)
    if ptrs is None or len(ptrs) != len(keep):
        ptrs = mod._sir_wptrs = tuple(t.data_ptr() for t in keep)      # constant while the pointer struct is cached
    key = (_weights_epoch[0], token, workspace.generation if workspace is not None else 0,
           tuple(map(_tensor_version, keep)), ptrs)
    return (hash(key) & 0xFFFFFFFFFFFFFFFF) or 1


class Workspace:
    """Grow-only device scratch, 256-byte aligned (torch's caching allocator aligns to 512).  ``generation`` counts the
    allocations: prepared weight layouts live inside the buffer, so a new buffer (even at the old address) invalidates
    them -- ``weights_version`` folds the generation in."""
    _generations = itertools.count(1)

    def __init__(self):
        self.buf = None
        self.generation = 0

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
            self.generation = next(Workspace._generations)
        return self.buf


def check_status(all_ranks=True):
    """Raise ``SirError`` if a GRU recurrence launched since the last check timed out in its inter-workgroup exchange
    (``sir_check_status``: its outputs were invalid) or ``sir_ce_loss`` met a label outside ``[0, num_classes)``.
    Host-synchronous on the current stream -- call it where the host waits anyway (end of an epoch, after a batch of
    predictions has been copied back).  In a data-parallel job the flag is MAX-reduced over the ranks first, so that
    EVERY rank raises (a rank that raised alone would leave the others blocked in the next collective until the RCCL
    timeout); every rank must therefore call it at the same point."""
    import torch.distributed as dist
    lib = _native.lib()
    rc = lib.sir_check_status(get_featurizer().handle, _native.current_stream_ptr())
    if all_ranks and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        flag = torch.tensor([1 if rc != _native.SIR_OK else 0], dtype=torch.int32, device="cuda")
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if rc == _native.SIR_OK and int(flag.item()):
            raise _native.SirError("sir_check_status failed on another rank of this job (a GRU recurrence timed out or a "
                                   "label was out of range there): this rank stops with it")
    _native.check(rc, "sir_check_status")


def _as_features(x):
    if x.dim() == 4:
        if x.shape[1] != 1:
            raise _native.SirError("input_channels must be 1")
        x = x[:, 0]
    if x.dim() != 3 or x.shape[1] != 64:
        raise _native.SirError(f"expected [B,64,T] or [B,1,64,T], got {tuple(x.shape)}")
    if x.shape[2] < 8:
        raise _native.SirError(f"need at least 8 frames, got {x.shape[2]} ({SHAPE_LIMITS})")
    return _f32c(x.contiguous(), "input")


def check_feature_batch(x, name, min_frames):
    """The host check of the functions that validate before any device call (``sir_amd.explain``, ``train_ops.adv_step``): ``x`` is
    a float32 tensor ``[B,64,T]`` or ``[B,1,64,T]`` with ``T >= min_frames``, else ``ValueError``.  Returns ``(B, T)``."""
    if not torch.is_tensor(x) or x.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 tensor [B,64,T] or [B,1,64,T]")
    sh = tuple(x.shape)
    if not ((len(sh) == 3 and sh[1] == 64) or (len(sh) == 4 and sh[1] == 1 and sh[2] == 64)) or sh[-1] < min_frames:
        raise ValueError(f"{name}: expected [B,64,T] or [B,1,64,T] with T >= {min_frames}, got {sh}")
    return sh[0], sh[-1]


def _as_lengths(lengths, bsz, t, device):
    """``lengths`` of a ragged call as an int32 device tensor [B].  A host list (or a CPU tensor) is validated here and now;
    a device tensor is validated by the kernels (bad rows come back NaN and ``check_status`` raises)."""
    if not torch.is_tensor(lengths):
        lengths = torch.as_tensor(list(lengths))
    if lengths.dim() != 1 or lengths.numel() != bsz:
        raise _native.SirError(f"lengths must hold one entry per clip: got shape {tuple(lengths.shape)} for a batch of {bsz}")
    if lengths.is_floating_point() or lengths.dtype == torch.bool:
        raise _native.SirError("lengths must be integers (frames per clip)")
    if not lengths.is_cuda:
        bad = [(i, int(v)) for i, v in enumerate(lengths.tolist()) if not 8 <= int(v) <= t]
        if bad:
            raise _native.SirError(f"lengths outside [8, {t}] (clip, frames): {bad[:8]}")
        lengths = lengths.to(device)
    return lengths.to(torch.int32).contiguous()


def model_infer(mod, x, workspace, want_argmax=False, debug=None, lengths=None):
    """eval-mode forward of ``CNNAudioGRU`` on the GPU -> logits [B, C] (and argmax int64 [B]).

    ``lengths`` (int tensor or list, frames per clip): the un-padded function (``sir_model_infer_ragged``) -- row b is
    what the model gives ``x[b:b+1, :, :lengths[b]]`` on its own; the columns behind a clip's length are never read as data."""
    _native.require_hip(x)
    x = _as_features(x)
    bsz, _, t = x.shape
    lib = _native.lib()
    h = get_featurizer().handle
    need = lib.sir_model_workspace_bytes(h, bsz, t, 0)
    if need == 0:
        raise _native.SirError(f"unsupported shape batch={bsz} frames={t} ({SHAPE_LIMITS})")
    if lengths is not None:
        lengths = _as_lengths(lengths, bsz, t, x.device)
    ws = workspace.get(need, x.device)
    w, keep = cached_weights(mod)
    logits = torch.empty((bsz, w.num_classes), dtype=torch.float32, device=x.device)
    amax = torch.empty((bsz,), dtype=torch.int64, device=x.device) if want_argmax else None
    lib.sir_model_set_weights_version(h, weights_version(mod, keep, workspace))
    if lengths is None:
        rc = lib.sir_model_infer(h, C.byref(w), x.data_ptr(), bsz, t, logits.data_ptr(),
                                 amax.data_ptr() if amax is not None else None, ws.data_ptr(), ws.numel(),
                                 _native.current_stream_ptr())
        _native.check(rc, "sir_model_infer")
    else:
        rc = lib.sir_model_infer_ragged(h, C.byref(w), x.data_ptr(), lengths.data_ptr(), bsz, t, logits.data_ptr(),
                                        amax.data_ptr() if amax is not None else None, ws.data_ptr(), ws.numel(),
                                        _native.current_stream_ptr())
        _native.check(rc, "sir_model_infer_ragged")
    if debug is not None:
        debug.update(stage_views(ws, bsz, t))
    del keep
    return (logits, amax) if want_argmax else logits


def model_embed(mod, x, workspace, lengths=None, want_logits=False, debug=None):
    """The forward of ``model_infer`` returning the utterance embeddings (``sir_model_embed``): the attention-pooled context,
    [B, 512] float32, raw and un-normalised -- what ``sir_amd.prototypes`` enrols and scores.  A row whose logits
    ``model_infer`` makes NaN (a non-finite feature, a bad ragged length) is all-NaN.  ``lengths`` as in ``model_infer``.
    ``want_logits=True`` -> ``(emb, logits, argmax)``, logits and argmax bit-identical to ``model_infer``'s; without it the
    classifier is not run."""
    _native.require_hip(x)
    x = _as_features(x)
    bsz, _, t = x.shape
    lib = _native.lib()
    h = get_featurizer().handle
    need = lib.sir_model_workspace_bytes(h, bsz, t, 0)
    if need == 0:
        raise _native.SirError(f"unsupported shape batch={bsz} frames={t} ({SHAPE_LIMITS})")
    if lengths is not None:
        lengths = _as_lengths(lengths, bsz, t, x.device)
    ws = workspace.get(need, x.device)
    w, keep = cached_weights(mod)
    emb = torch.empty((bsz, 512), dtype=torch.float32, device=x.device)
    logits = torch.empty((bsz, w.num_classes), dtype=torch.float32, device=x.device) if want_logits else None
    amax = torch.empty((bsz,), dtype=torch.int64, device=x.device) if want_logits else None
    lib.sir_model_set_weights_version(h, weights_version(mod, keep, workspace))
    rc = lib.sir_model_embed(h, C.byref(w), x.data_ptr(), lengths.data_ptr() if lengths is not None else None, bsz, t,
                             emb.data_ptr(), logits.data_ptr() if want_logits else None, amax.data_ptr() if want_logits else None,
                             ws.data_ptr(), ws.numel(), _native.current_stream_ptr())
    _native.check(rc, "sir_model_embed")
    if debug is not None:
        debug.update(stage_views(ws, bsz, t))
    del keep
    return (emb, logits, amax) if want_logits else emb


def classify(logits, k=3, inv_temperature=None, want_probs=False):
    """Softmax and top-k of a batch of logits in one ``sir_classify`` launch -> ``(topk_idx int32 [B, k], topk_prob float32
    [B, k])``, classes by descending logit (equal logits: the lower index first), so ``topk_idx[:, 0]`` is the argmax
    ``model_infer`` returns and ``topk_prob[:, 0]`` the confidence.  ``inv_temperature``: None, a positive number or a device
    scalar (``metrics.fit_temperature``) that scales the logits first.  A row with a NaN or an infinity comes back as -1 / NaN.
    ``want_probs=True`` appends the full softmax [B, C]."""
    from .metrics import _inv_temperature_tensor
    _native.require_hip(logits)
    if logits.dim() != 2 or logits.shape[0] < 1 or not 1 <= logits.shape[1] <= 64:
        raise _native.SirError(f"logits must be [rows >= 1, classes in 1..64], got {tuple(logits.shape)}")
    logits = _f32c(logits.contiguous(), "logits")
    bsz, ncls = logits.shape
    if isinstance(k, bool) or not hasattr(k, "__index__") or not 1 <= int(k) <= min(8, ncls):
        raise _native.SirError(f"k must be an integer in [1, min(8, {ncls})], got {k!r}")
    k = int(k)
    beta = _inv_temperature_tensor(inv_temperature, logits.device)
    idx = torch.empty((bsz, k), dtype=torch.int32, device=logits.device)
    prob = torch.empty((bsz, k), dtype=torch.float32, device=logits.device)
    probs = torch.empty_like(logits) if want_probs else None
    rc = _native.lib().sir_classify(get_featurizer().handle, logits.data_ptr(), bsz, ncls,
                                    beta.data_ptr() if beta is not None else None, k,
                                    probs.data_ptr() if probs is not None else None, idx.data_ptr(), prob.data_ptr(),
                                    _native.current_stream_ptr())
    _native.check(rc, "sir_classify")
    return (idx, prob, probs) if want_probs else (idx, prob)


def stage_views(ws, bsz, t):
    """Views of the intermediate buffers inside the workspace (for stage-level parity tests)."""
    lib = _native.lib()
    offs = (C.c_size_t * 16)()
    n = lib.sir_model_workspace_offsets(get_featurizer().handle, bsz, t, 0, offs, 16)
    if n <= 0:
        raise _native.SirError("sir_model_workspace_offsets failed")
    wp1, wp2 = t // 2, t // 4
    s = wp2 // 2
    shapes = {"conv1": (bsz, 32, wp1, 32), "conv2": (bsz, 16, wp2, 64), "gru_in": (bsz, s, 1024),
              "gi": (bsz * s, 1536), "gru_l0": (bsz, s, 512), "gru_l1": (bsz, s, 512), "ctx": (bsz, 512)}
    out = {}
    for i, name in enumerate(WS_NAMES):
        shp = shapes[name]
        numel = 1
        for v in shp:
            numel *= v
        out[name] = ws[offs[i]: offs[i] + 4 * numel].view(torch.float32).view(shp)
    return out


_PAD_TABLES = ("e0", "d1", "d3", "rows", "tab2", "tab3", "record", "nonfinite")


def _pad_table_offsets(bsz, t):
    """``sir_model_infer_table_offsets`` (include/sir_hip.h) as a dict: the int offset of every pad-skip table inside its workspace
    slot, ``ints`` (the slot's size) and ``base`` (the slot's byte offset in the workspace)"""
    lib = _native.lib()
    vals, offs = (C.c_size_t * 10)(), (C.c_size_t * 16)()
    if lib.sir_model_infer_table_offsets(None, bsz, t, vals, 10) != 10:
        raise _native.SirError("sir_model_infer_table_offsets failed")
    if lib.sir_model_workspace_offsets(None, bsz, t, 0, offs, 16) <= vals[9]:
        raise _native.SirError("sir_model_workspace_offsets failed")
    out = dict(zip(_PAD_TABLES + ("ints",), vals))
    out["base"] = offs[vals[9]]
    return out


def pad_skip_tables(ws, bsz, t):
    """The pad-skip tables the last padded ``model_infer`` call on ``ws`` left (csrc/infer_tables.h), on the host: ``e0`` [B],
    ``d1`` and ``d3`` [B + 1] (the template utterance last), ``nonfinite`` [B], ``rows`` (the listed rows of the layer-0 projection,
    by the count word) and the conv2 / conv3 task lists (``Wino2Geo::ctab`` in csrc/wino2_geo.h) as int32 arrays ``tab2`` / ``tab3``
    of shape [n, 2]: the two words of each listed task."""
    o = _pad_table_offsets(bsz, t)
    n = bsz + 1
    tab = ws[o["base"]: o["base"] + 4 * o["ints"]].view(torch.int32).cpu()
    out = {name: tab[o[name]: o[name] + cnt] for name, cnt in (("e0", bsz), ("d1", n), ("d3", n), ("nonfinite", bsz))}
    out["rows"] = tab[o["rows"] + 1: o["rows"] + 1 + int(tab[o["rows"]])]
    for name in ("tab2", "tab3"):
        cnt = int(tab[o[name]])
        out[name] = tab[o[name] + 2: o[name] + 2 + 2 * cnt].view(cnt, 2)
    return out


def proj_tile_record(ws, bsz, t):
    """What the latest row-list input projection of a ``model_infer`` call on ``ws`` read and chose (two ints behind the pad-skip
    tables, written by workgroup 0 of ``gemm_nt_f16x3_gather_kernel``): ``(rows, tile)`` -- the listed row count and the tile
    height, 96 / 128 / 160 rows.  A padded call leaves layer 0's record, a ragged call layer 1's (K = 512, the same row list)."""
    o = _pad_table_offsets(bsz, t)
    rec = ws[o["base"] + 4 * o["record"]: o["base"] + 4 * o["record"] + 8].view(torch.int32).cpu()
    return int(rec[0]), int(rec[1])
