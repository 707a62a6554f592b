"""Intents enrolled from examples: a bank of class prototypes over the utterance embeddings, and the prototype head.

``CNNAudioGRU.embed`` gives the 512-float attention-pooled context of every utterance (``sir_model_embed``).  A
``PrototypeBank`` sums the unit-normalised embeddings of each class's examples on the device (``sir_proto_accumulate``: one pass,
no backward), turns the sums into unit prototypes (``sir_proto_finalize``) and scores a batch against them by cosine similarity
in one launch (``sir_proto_score``): the k most similar classes, their similarities, a softmax over ``scale * similarity`` and the
nearest prototype.  Rejection is by distance: ``min_similarity`` marks the rows whose best cosine is below it.

The state of a bank after enrolling a set of rows carries the same bits however the rows were cut into ``enroll`` calls, and a
saved bank (one ``.npz`` of ``sum``, ``count``, ``skipped`` and ``names``: data only) continues enrolling to the same bits.
Only pointer plumbing lives here; there is no CPU path for the arithmetic.
"""
import collections

import numpy as np
import torch

from . import _native
from .featurizer import get_featurizer

DIM = 512
MAX_PROTOTYPES = 4096
HEADER_BYTES = 64

ProtoScores = collections.namedtuple("ProtoScores", "classes sims probs nearest rejected")
ProtoScores.__doc__ = """``PrototypeBank.score``'s result, device tensors: ``classes`` int32 [B, k] (indices into ``bank.names``, -1 = no
such rank / a row that could not be scored), ``sims`` float32 [B, k] (the class's cosine), ``probs`` float32 [B, k], ``nearest``
int32 [B] (the prototype row of rank 0) and ``rejected`` bool [B] (None without ``min_similarity``)."""


def _emb2d(embeddings):
    _native.require_hip(embeddings)
    if embeddings.dim() != 2 or embeddings.shape[1] != DIM or embeddings.shape[0] < 1 or embeddings.dtype != torch.float32:
        raise _native.SirError(f"embeddings must be float32 [rows >= 1, {DIM}], got {tuple(embeddings.shape)} {embeddings.dtype}")
    return embeddings.contiguous()


class PrototypeBank:
    """``names``: the classes the bank starts with (more are added by ``enroll``, up to 4096).  ``exemplars=False``: one
    prototype per class, the normalised mean of its examples' unit embeddings (a nearest-class-mean head).  ``exemplars=True``:
    every enrolled row is kept as its own unit-norm prototype with its class (1-nearest-neighbour; at most 4096 rows).
    ``scale`` (None, a positive number or a device scalar, e.g. ``fit_scale``'s) is what ``score`` uses when it is given none."""

    def __init__(self, names=(), exemplars=False):
        self.names = []
        self._index = {}
        self.exemplars = bool(exemplars)
        self.scale = None
        self._row_class = []                 # exemplars: the class of every stored row
        self._state = None                   # device state of sir_proto_*, laid out for _state_rows rows
        self._state_rows = 0
        self._host = {"sum": np.zeros((0, DIM), np.float64), "count": np.zeros((0,), np.int64), "skipped": 0}
        self._protos = None
        for n in names:
            self._add_name(n)

    # ---- names -------------------------------------------------------------------------------------------------------------
    def _add_name(self, name):
        if not isinstance(name, str) or not name:
            raise ValueError(f"a class name is a non-empty string, got {name!r}")
        if name in self._index:
            raise ValueError(f"class {name!r} is named twice")
        if len(self.names) >= MAX_PROTOTYPES:
            raise _native.SirError(f"a bank holds at most {MAX_PROTOTYPES} classes")
        self._index[name] = len(self.names)
        self.names.append(name)

    def _resolve_labels(self, labels_or_names, n_rows):
        """One class index per row from names (unseen ones extend the bank) or integers (-1 = ignore the row; anything else
        outside the bank is passed on and skipped by the kernel).  The bank's names are extended only when every label is good."""
        if torch.is_tensor(labels_or_names):
            labels_or_names = labels_or_names.tolist()
        labels = list(labels_or_names)
        if len(labels) != n_rows:
            raise ValueError(f"{len(labels)} labels for {n_rows} embeddings")
        if all(isinstance(v, str) for v in labels):
            new = []
            for v in labels:
                if v not in self._index and v not in new:
                    if not v:
                        raise ValueError("a class name is a non-empty string")
                    new.append(v)
            if len(self.names) + len(new) > MAX_PROTOTYPES:
                raise _native.SirError(f"a bank holds at most {MAX_PROTOTYPES} classes: {len(self.names)} named, {len(new)} new")
            for v in new:
                self._add_name(v)
            return [self._index[v] for v in labels]
        if any(isinstance(v, (str, bool)) or not hasattr(v, "__index__") for v in labels):
            raise ValueError("labels are all names or all integers")
        return [int(v) for v in labels]

    # ---- the device state --------------------------------------------------------------------------------------------------
    @property
    def n_rows(self):
        """rows of the state: the classes, or with ``exemplars=True`` the stored exemplars"""
        return len(self._row_class) if self.exemplars else len(self.names)

    def _views(self, state, rows):
        count = state[HEADER_BYTES: HEADER_BYTES + 8 * rows].view(torch.int64)
        base = HEADER_BYTES + 8 * rows
        return state[8:16].view(torch.int64), count, state[base: base + 8 * DIM * rows].view(torch.float64).view(rows, DIM)

    def _ensure_state(self, device=None):
        """The device state laid out for ``n_rows`` rows: a bank that grew (or was loaded) gets a new buffer, and its sums and
        counts are copied over bit for bit."""
        rows = self.n_rows
        if rows < 1:
            raise _native.SirError("the bank is empty: enrol something first")
        if self._state is not None and self._state_rows == rows:
            return self._state
        if device is None:
            device = self._state.device if self._state is not None else torch.device("cuda", torch.cuda.current_device())
        lib = _native.lib()
        need = lib.sir_proto_state_bytes(rows)
        state = torch.empty((need,), dtype=torch.uint8, device=device)
        _native.check(lib.sir_proto_reset(get_featurizer().handle, state.data_ptr(), need, rows, None, _native.current_stream_ptr()),
                      "sir_proto_reset")
        skipped, count, total = self._views(state, rows)
        if self._state is not None:
            old_skipped, old_count, old_total = self._views(self._state, self._state_rows)
            n = min(rows, self._state_rows)
            skipped.copy_(old_skipped)
            count[:n].copy_(old_count[:n])
            total[:n].copy_(old_total[:n])
        elif self._host["count"].shape[0]:
            n = min(rows, self._host["count"].shape[0])
            skipped.fill_(int(self._host["skipped"]))
            count[:n].copy_(torch.from_numpy(self._host["count"][:n]).to(device))
            total[:n].copy_(torch.from_numpy(self._host["sum"][:n]).to(device))
        self._state, self._state_rows = state, rows
        self._host = {"sum": np.zeros((0, DIM), np.float64), "count": np.zeros((0,), np.int64), "skipped": 0}
        return state

    def state_arrays(self):
        """``{"sum": float64 [rows, 512], "count": int64 [rows], "skipped": int}`` on the host: what ``save`` writes."""
        rows = self.n_rows
        if self._state is None:
            h = self._host
            total, count = np.zeros((rows, DIM), np.float64), np.zeros((rows,), np.int64)
            n = min(rows, h["count"].shape[0])
            total[:n], count[:n] = h["sum"][:n], h["count"][:n]
            return {"sum": total, "count": count, "skipped": int(h["skipped"])}
        if self._state_rows != rows:
            self._ensure_state()
        skipped, count, total = self._views(self._state, rows)
        return {"sum": total.cpu().numpy(), "count": count.cpu().numpy(), "skipped": int(skipped.item())}

    def state_tensor(self):
        """The raw device state (``sir_proto_state_bytes(n_rows)`` bytes, include/sir_hip.h lays it out)."""
        return self._ensure_state()

    # ---- enrolment ---------------------------------------------------------------------------------------------------------
    def enroll(self, embeddings, labels_or_names):
        """Add rows of ``embeddings`` [B, 512] (``CNNAudioGRU.embed``) to their classes.  ``labels_or_names``: one name per row
        (unseen names extend the bank, up to 4096) or one class index per row (-1 = ignore).  A row with a NaN, an infinity or
        norm zero, or with an index outside the bank, is skipped and counted in ``state_arrays()["skipped"]``.  -> self."""
        if embeddings.dim() != 2:
            raise _native.SirError(f"embeddings must be [rows, {DIM}], got {tuple(embeddings.shape)}")
        ids = self._resolve_labels(labels_or_names, embeddings.shape[0])
        emb = _emb2d(embeddings)
        if self.exemplars:                                       # a row of its own for every row with a class of the bank
            first, rows = len(self._row_class), []
            for c in ids:
                if 0 <= c < len(self.names):
                    rows.append(first + len(rows))
                else:
                    rows.append(-1)
            n_new = sum(1 for r in rows if r >= 0)
            if first + n_new > MAX_PROTOTYPES:
                raise _native.SirError(f"an exemplar bank holds at most {MAX_PROTOTYPES} rows: {first} stored, {n_new} new")
            self._row_class.extend(c for c, r in zip(ids, rows) if r >= 0)
            ids = rows
        elif not self.names:
            raise _native.SirError("the bank has no classes: enrol by name, or name the classes first")
        self._protos = None
        rows = self.n_rows
        if rows < 1:                                             # (exemplars: nothing but ignored rows so far)
            self._host["skipped"] = int(self._host["skipped"]) + len(ids)
            return self
        state = self._ensure_state(emb.device)
        labels = torch.tensor(ids, dtype=torch.int64, device=emb.device)
        rc = _native.lib().sir_proto_accumulate(get_featurizer().handle, state.data_ptr(), state.numel(), rows, emb.data_ptr(),
                                                labels.data_ptr(), emb.shape[0], _native.current_stream_ptr())
        _native.check(rc, "sir_proto_accumulate")
        return self

    def remove(self, name):
        """Clear a class: its sum and count go back to zero (``sir_proto_reset`` with a mask; an exemplar bank clears the class's
        rows).  The name keeps its index, so the other classes keep theirs; the class is absent from ``score`` until it is
        enrolled again."""
        if name not in self._index:
            raise KeyError(name)
        self._protos = None
        c, rows = self._index[name], self.n_rows
        if rows < 1:
            return self
        mask = np.zeros((rows,), np.uint8)
        if self.exemplars:
            mask[[r for r, rc in enumerate(self._row_class) if rc == c]] = 1
        else:
            mask[c] = 1
        if not mask.any():
            return self
        state = self._ensure_state()
        dmask = torch.from_numpy(mask).to(state.device)
        rc = _native.lib().sir_proto_reset(get_featurizer().handle, state.data_ptr(), state.numel(), rows, dmask.data_ptr(),
                                           _native.current_stream_ptr())
        _native.check(rc, "sir_proto_reset")
        return self

    # ---- prototypes and scores ---------------------------------------------------------------------------------------------
    def prototypes(self):
        """``(protos float32 [rows, 512], live uint8 [rows], proto_class int32 [rows] or None)`` on the device, finalised
        (``sir_proto_finalize``) and cached until the bank changes.  ``proto_class`` is None when row = class."""
        if self._protos is None:
            state = self._ensure_state()
            rows = self.n_rows
            protos = torch.empty((rows, DIM), dtype=torch.float32, device=state.device)
            live = torch.empty((rows,), dtype=torch.uint8, device=state.device)
            rc = _native.lib().sir_proto_finalize(get_featurizer().handle, state.data_ptr(), state.numel(), rows, protos.data_ptr(),
                                                  live.data_ptr(), _native.current_stream_ptr())
            _native.check(rc, "sir_proto_finalize")
            pclass = lut = None
            if self.exemplars:                                   # classes that own rows, renumbered densely in name order
                present = sorted(set(self._row_class))
                dense = {c: i for i, c in enumerate(present)}
                pclass = torch.tensor([dense[c] for c in self._row_class], dtype=torch.int32, device=state.device)
                lut = torch.tensor(present, dtype=torch.int32, device=state.device)
            self._protos = (protos, live, pclass, lut)
        return self._protos[:3]

    def score(self, embeddings, k=3, scale=None, min_similarity=None):
        """``embeddings`` [B, 512] against the bank in one ``sir_proto_score`` launch -> ``ProtoScores``: the ``k`` (1..8) most
        similar classes of every row (equal similarities: the lower class first), their cosine, the softmax of ``scale *
        similarity`` over the classes that have a prototype (``scale``: None = the bank's ``scale``, a positive number or a
        device scalar) and the nearest prototype.  ``min_similarity`` adds ``rejected``: the best cosine is below it (or NaN)."""
        from .metrics import _inv_temperature_tensor
        emb = _emb2d(embeddings)
        if isinstance(k, bool) or not hasattr(k, "__index__") or not 1 <= int(k) <= 8:
            raise _native.SirError(f"k must be an integer in [1, 8], got {k!r}")
        k = int(k)
        protos, live, pclass = self.prototypes()
        lut = self._protos[3]
        beta = _inv_temperature_tensor(self.scale if scale is None else scale, emb.device)
        bsz, rows = emb.shape[0], protos.shape[0]
        n_classes = rows if pclass is None else int(lut.numel())
        classes = torch.empty((bsz, k), dtype=torch.int32, device=emb.device)
        sims = torch.empty((bsz, k), dtype=torch.float32, device=emb.device)
        probs = torch.empty((bsz, k), dtype=torch.float32, device=emb.device)
        nearest = torch.empty((bsz,), dtype=torch.int32, device=emb.device)
        rc = _native.lib().sir_proto_score(get_featurizer().handle, emb.data_ptr(), bsz, protos.data_ptr(), live.data_ptr(),
                                           pclass.data_ptr() if pclass is not None else None, rows, n_classes,
                                           beta.data_ptr() if beta is not None else None, k, None, classes.data_ptr(),
                                           sims.data_ptr(), probs.data_ptr(), nearest.data_ptr(), _native.current_stream_ptr())
        _native.check(rc, "sir_proto_score")
        if lut is not None:                                      # dense class numbers back to indices into names
            classes = torch.where(classes >= 0, lut[classes.clamp(min=0).long()], classes)
        rejected = None
        if min_similarity is not None:
            rejected = ~(sims[:, 0] >= float(min_similarity))
        return ProtoScores(classes, sims, probs, nearest, rejected)

    # ---- the bank file -----------------------------------------------------------------------------------------------------
    def save(self, path):
        """One ``.npz`` of ``sum``, ``count``, ``skipped`` and ``names`` (an exemplar bank adds ``row_class``): data only."""
        a = self.state_arrays()
        extra = {"row_class": np.asarray(self._row_class, np.int32)} if self.exemplars else {}
        with open(path, "wb") as f:
            np.savez(f, sum=a["sum"], count=a["count"], skipped=np.int64(a["skipped"]), names=np.asarray(self.names, dtype=np.str_),
                     **extra)

    @classmethod
    def from_proxies(cls, head):
        """A mean bank of a trained ``ProxyHead``: one class per proxy, count 1, its sum the unit proxy (normalised in float64),
        so ``score`` ranks against the centres the loss trained.  No device call; rows of norm zero or not finite stay empty."""
        bank = cls(head.names)
        p = head.proxies.detach().to("cpu", torch.float64).numpy()
        norm = np.sqrt((p * p).sum(axis=1))
        ok = np.isfinite(p).all(axis=1) & (norm > 0.0)
        bank._host = {"sum": np.where(ok[:, None], p / np.where(ok, norm, 1.0)[:, None], 0.0),
                      "count": ok.astype(np.int64), "skipped": 0}
        return bank

    @classmethod
    def load(cls, path):
        """A saved bank; enrolling into it continues to the bits of an uninterrupted enrolment."""
        with np.load(path, allow_pickle=False) as z:
            names = [str(n) for n in z["names"].tolist()]
            bank = cls(names, exemplars="row_class" in z.files)
            total, count = np.ascontiguousarray(z["sum"], np.float64), np.ascontiguousarray(z["count"], np.int64)
            if bank.exemplars:
                bank._row_class = [int(c) for c in z["row_class"].tolist()]
                if any(not 0 <= c < len(names) for c in bank._row_class):
                    raise ValueError("the bank file's row_class names a class it does not have")
            if total.shape != (bank.n_rows, DIM) or count.shape != (bank.n_rows,):
                raise ValueError(f"the bank file holds sum {total.shape} / count {count.shape} for {bank.n_rows} rows")
            bank._host = {"sum": total, "count": count, "skipped": int(z["skipped"])}
        return bank


def fit_scale(bank, embeddings, labels, iters=20):
    """The ``scale`` that minimises the mean NLL of ``softmax(scale * similarity)`` on a held-out split, by
    ``metrics.fit_temperature`` on the similarities (no kernel of its own).  That call serves at most 64 classes, and the
    similarities are the class scores only when every class has exactly one live prototype: a mean bank of at most 64 classes,
    all enrolled.  -> ``fit_temperature``'s device tensor; ``bank.scale = fit_scale(...)`` makes it the bank's default.  (The fit
    clamps to [1/64, 64].)"""
    from . import metrics
    if bank.exemplars or len(bank.names) > metrics.MAX_CLASSES:
        raise _native.SirError(f"fit_scale serves a mean bank of at most {metrics.MAX_CLASSES} classes")
    emb = _emb2d(embeddings)
    protos, live, _ = bank.prototypes()
    if not bool(live.all().item()):
        raise _native.SirError("fit_scale needs every class of the bank enrolled")
    bsz, rows = emb.shape[0], protos.shape[0]
    sims = torch.empty((bsz, rows), dtype=torch.float32, device=emb.device)
    scratch_i = torch.empty((bsz, 1), dtype=torch.int32, device=emb.device)
    scratch_f = torch.empty((2, bsz, 1), dtype=torch.float32, device=emb.device)
    rc = _native.lib().sir_proto_score(get_featurizer().handle, emb.data_ptr(), bsz, protos.data_ptr(), None, None, rows, rows, None, 1,
                                       sims.data_ptr(), scratch_i.data_ptr(), scratch_f[0].data_ptr(), scratch_f[1].data_ptr(), None,
                                       _native.current_stream_ptr())
    _native.check(rc, "sir_proto_score")
    return metrics.fit_temperature(sims, labels, iters=iters)


class _ProxyLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, proxies, labels, scale, margin, head):
        lib = _native.lib()
        _native.require_hip(emb, proxies, labels)
        if proxies.dim() != 2 or proxies.shape[1] != DIM or proxies.dtype != torch.float32 or not 1 <= proxies.shape[0] <= MAX_PROTOTYPES:
            raise _native.SirError(f"proxies must be float32 [1..{MAX_PROTOTYPES}, {DIM}], got {tuple(proxies.shape)} {proxies.dtype}")
        emb, proxies = _emb2d(emb), proxies.contiguous()
        labels = labels.to(torch.int64).contiguous()
        bsz, n = emb.shape[0], proxies.shape[0]
        if labels.dim() != 1 or labels.numel() != bsz:
            raise _native.SirError(f"{labels.numel()} labels for {bsz} embeddings")
        need = lib.sir_proxy_loss_workspace_bytes(bsz, n)
        ws = head._workspace(need, emb.device)
        loss = torch.empty((), dtype=torch.float32, device=emb.device)
        demb = torch.empty_like(emb) if ctx.needs_input_grad[0] else None
        dprox = torch.empty_like(proxies) if ctx.needs_input_grad[1] else None
        rc = lib.sir_proxy_loss(get_featurizer().handle, emb.data_ptr(), proxies.data_ptr(), labels.data_ptr(), bsz, n, float(scale),
                                float(margin), loss.data_ptr(), demb.data_ptr() if demb is not None else None,
                                dprox.data_ptr() if dprox is not None else None, 1.0, ws.data_ptr(), ws.numel(),
                                _native.current_stream_ptr())
        _native.check(rc, "sir_proxy_loss")
        ctx.demb, ctx.dprox = demb, dprox
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        # loss.backward() passes 1.0; a general scalar (a loss weight) is applied by the two multiplies below
        return (ctx.demb * grad_out if ctx.demb is not None else None, ctx.dprox * grad_out if ctx.dprox is not None else None,
                None, None, None, None)


class ProxyHead(torch.nn.Module):
    """The cosine-proxy loss on the embeddings (``sir_proxy_loss``): one learned centre per class, ``proxies`` float32
    ``[n_classes, 512]`` (normal init from ``seed``; they need not stay unit), and ``head(emb, labels)`` = the mean over the
    labelled rows of ``-log softmax(scale * (cos(emb, proxy_k) - margin * [k == label]))[label]`` -- normalised softmax with
    ``margin == 0``, AM-softmax / CosFace with a margin.  Labels as for ``fused_cross_entropy`` (-100 ignores a row).  Both
    gradients are written in the forward, as ``fused_cross_entropy`` writes its own.  ``emb`` is
    ``model.forward_with_embedding(x)[1]``; ``PrototypeBank.from_proxies(head)`` turns the trained centres into a bank."""

    def __init__(self, n_classes, names=None, scale=16.0, margin=0.0, seed=0):
        super().__init__()
        n_classes = int(n_classes)
        if not 1 <= n_classes <= MAX_PROTOTYPES:
            raise ValueError(f"n_classes={n_classes} outside [1, {MAX_PROTOTYPES}]")
        scale, margin = float(scale), float(margin)
        if not (scale > 0.0 and np.isfinite(scale)):
            raise ValueError("scale must be positive and finite")
        if not (margin >= 0.0 and np.isfinite(margin)):
            raise ValueError("margin must be finite and >= 0")
        names = [f"class_{i}" for i in range(n_classes)] if names is None else [str(n) for n in names]
        if len(names) != n_classes or len(set(names)) != n_classes or any(not n for n in names):
            raise ValueError(f"names must be {n_classes} distinct non-empty strings")
        self.names, self.scale, self.margin = names, scale, margin
        gen = torch.Generator().manual_seed(int(seed))
        self.proxies = torch.nn.Parameter(torch.randn(n_classes, DIM, generator=gen, dtype=torch.float32))
        self._ws = None

    def _workspace(self, nbytes, device):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        return self._ws

    def forward(self, emb, labels):
        return _ProxyLoss.apply(emb, self.proxies, labels, self.scale, self.margin, self)

    @torch.no_grad()
    def init_from_bank(self, bank):
        """Start the centres from an enrolled mean bank: row c = the unit mean of class c (float64 on the host, no device
        call); the bank must name the head's classes in order and have every one enrolled.  -> self."""
        if bank.exemplars:
            raise ValueError("init_from_bank takes a mean bank (exemplars=False)")
        if list(bank.names) != list(self.names):
            raise ValueError("the bank's names are not the head's")
        a = bank.state_arrays()
        norm = np.sqrt((a["sum"] ** 2).sum(axis=1))
        if not ((a["count"] > 0) & np.isfinite(norm) & (norm > 0.0)).all():
            raise ValueError("init_from_bank needs every class of the bank enrolled")
        unit = torch.from_numpy((a["sum"] / norm[:, None]).astype(np.float32))
        self.proxies.copy_(unit.to(self.proxies.device))
        return self
