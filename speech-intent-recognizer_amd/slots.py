"""Slot heads: one logit row read as several independent softmax segments (DESIGN.md section 4 "Slot heads").

Fluent Speech Commands labels a clip with an action, an object and a location; the reference joins the first two into
one class and drops the third.  Here the model is unchanged -- ``fc`` still writes up to 64 logits per utterance -- and a
``SlotSpec`` says which columns of that row belong to which slot: FSC's 6 actions + 14 objects + 4 locations are 24 of
them.  Loss (``sir_ce_loss_slots``), classification with a joint confidence (``sir_classify_slots``) and the evaluation
counts with exact match (``sir_eval_accumulate_slots``) then work per segment, with the arithmetic of their single-head
relatives.  Everything here validates on the host before the first device call.
"""
import ctypes as C
import json
import logging

import numpy as np

from . import _native, metrics

logger = logging.getLogger(__name__)

IGNORE = -100
MAX_SLOTS = 8
MAX_CLASSES = 64
JOINT_SLOTS_CORRECT = MAX_SLOTS + 1
_JOINT_INT_FIELDS = ("n", "exact_match", "slots_correct", "bin_count", "bin_correct", "n_excluded")
_JOINT_FLOAT_FIELDS = ("nll_sum", "bin_conf_sum")


def check_sizes(sizes):
    """The layout rules of include/sir_hip.h: 1..8 widths, each >= 1, adding up to at most 64 -> tuple of ints."""
    try:
        out = tuple(sizes)
    except TypeError:
        raise ValueError(f"slot sizes must be a sequence of integers, got {sizes!r}") from None
    if not 1 <= len(out) <= MAX_SLOTS:
        raise ValueError(f"a slot layout has 1..{MAX_SLOTS} slots, got {len(out)}")
    for s in out:
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or s < 1:
            raise ValueError(f"every slot width must be an integer >= 1, got {s!r}")
    if sum(out) > MAX_CLASSES:
        raise ValueError(f"the slot widths add up to {sum(out)}, at most {MAX_CLASSES} logits exist")
    return tuple(int(s) for s in out)


def starts_of(sizes):
    return tuple(int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]]))


class SlotSpec:
    """Which logit columns belong to which slot, and what their classes are called.

    ``columns``: the slot names, in logit order.  ``vocab``: per column the list of its values; value ``j`` of column ``g``
    is logit column ``starts[g] + j``."""

    def __init__(self, columns, vocab):
        columns = [str(c) for c in columns]
        if len(set(columns)) != len(columns):
            raise ValueError(f"slot columns must be distinct, got {columns}")
        if isinstance(vocab, dict):
            missing = [c for c in columns if c not in vocab]
            if missing:
                raise ValueError(f"no vocabulary for slot columns {missing}")
            vocab = [vocab[c] for c in columns]
        vocab = [[str(v) for v in vs] for vs in vocab]
        if len(vocab) != len(columns):
            raise ValueError(f"{len(columns)} slot columns but {len(vocab)} vocabularies")
        for c, vs in zip(columns, vocab):
            if len(set(vs)) != len(vs):
                raise ValueError(f"the vocabulary of slot {c!r} holds a value twice")
        self.sizes = check_sizes([len(vs) for vs in vocab])
        self.columns = tuple(columns)
        self.vocab = tuple(tuple(vs) for vs in vocab)
        self.starts = starts_of(self.sizes)
        self.total = int(sum(self.sizes))
        self._index = [{v: j for j, v in enumerate(vs)} for vs in self.vocab]
        self._warned = set()

    @property
    def n_slots(self):
        return len(self.sizes)

    @classmethod
    def from_sizes(cls, sizes):
        """A spec with numbered names, for callers that only have widths."""
        sizes = check_sizes(sizes)
        return cls([f"slot{g}" for g in range(len(sizes))], [[str(j) for j in range(s)] for s in sizes])

    @classmethod
    def from_csv(cls, csv, columns=("action", "object", "location")):
        """A sorted vocabulary per column of the CSV file (or DataFrame) ``csv``."""
        data = csv
        if isinstance(csv, (str, bytes)) or hasattr(csv, "__fspath__"):
            import pandas as pd
            data = pd.read_csv(csv)
        missing = [c for c in columns if c not in data.columns]
        if missing:
            raise ValueError(f"the CSV has no column(s) {missing}")
        return cls(columns, [sorted({str(v) for v in data[c]}) for c in columns])

    def to_dict(self):
        return {"columns": list(self.columns), "vocab": {c: list(vs) for c, vs in zip(self.columns, self.vocab)}}

    def save(self, path):
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=2)

    @classmethod
    def load(cls, path):
        with open(path, "r") as f:
            d = json.load(f)
        if not isinstance(d, dict) or "columns" not in d or "vocab" not in d:
            raise ValueError(f"{path}: not a slot map (needs 'columns' and 'vocab')")
        return cls(d["columns"], d["vocab"])

    def __eq__(self, other):
        return isinstance(other, SlotSpec) and self.columns == other.columns and self.vocab == other.vocab

    def encode(self, dataframe):
        """-> int64 numpy [N, G]: per row the slot-local index of each column's value; an unknown value becomes -100 (left out of
        that slot's loss and counts) and is logged once per column."""
        missing = [c for c in self.columns if c not in dataframe.columns]
        if missing:
            raise ValueError(f"the data has no column(s) {missing}")
        out = np.empty((len(dataframe), self.n_slots), dtype=np.int64)
        for g, c in enumerate(self.columns):
            index = self._index[g]
            col = [index.get(str(v), IGNORE) for v in dataframe[c]]
            out[:, g] = col
            if IGNORE in col and c not in self._warned:
                self._warned.add(c)
                unknown = sorted({str(v) for v in dataframe[c] if str(v) not in index})
                logger.warning(f"slot {c!r}: {len(unknown)} unknown value(s), e.g. {unknown[:3]}; such rows are ignored in this slot")
        return out

    def decode(self, idx_row):
        """Slot-local indices [G] -> {column: value}; an index outside the vocabulary (-100, -1) gives ``"Unknown"``."""
        idx_row = [int(v) for v in idx_row]
        if len(idx_row) != self.n_slots:
            raise ValueError(f"{len(idx_row)} indices for {self.n_slots} slots")
        return {c: (vs[i] if 0 <= i < len(vs) else "Unknown") for c, vs, i in zip(self.columns, self.vocab, idx_row)}

    def reference_label(self, decoded):
        """The reference's own label of a clip, ``action + '_' + object`` (scripts/preprocess_fsc.py), when the spec has both
        columns; None otherwise."""
        if "action" in self.columns and "object" in self.columns:
            return f"{decoded['action']}_{decoded['object']}"
        return None


def _as_spec(spec):
    return spec if isinstance(spec, SlotSpec) else SlotSpec.from_sizes(spec)


def _sizes_array(spec):
    return (C.c_int32 * spec.n_slots)(*spec.sizes)


def check_weights(weights, n_slots):
    """None or one finite weight >= 0 per slot -> None or a list of floats."""
    if weights is None:
        return None
    w = [float(v) for v in weights]
    if len(w) != n_slots:
        raise ValueError(f"{len(w)} slot weights for {n_slots} slots")
    for v in w:
        if not (v >= 0.0 and v != float("inf")):
            raise ValueError(f"slot weights must be finite and >= 0, got {v!r}")
    return w


def _check_smoothing(eps):
    eps = float(eps)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1), got {eps!r}")
    return eps


def _check_logits(logits, spec):
    import torch
    if not torch.is_tensor(logits) or logits.dim() != 2 or logits.dtype != torch.float32 or logits.shape[0] < 1:
        raise ValueError("logits must be a float32 tensor [rows >= 1, classes]")
    if logits.shape[1] != spec.total:
        raise ValueError(f"logits have {logits.shape[1]} columns, the slot layout {spec.sizes} needs {spec.total}")


def _check_labels(labels, logits, spec, name="labels"):
    import torch
    if not torch.is_tensor(labels) or labels.dtype != torch.int64 or tuple(labels.shape) != (logits.shape[0], spec.n_slots):
        raise ValueError(f"{name} must be an int64 tensor [{logits.shape[0]}, {spec.n_slots}] (one column per slot)")


def check_inv_temperature(inv_temperature, n_slots):
    """None, a positive number (all slots), one positive number per slot, or a float32 device tensor [n_slots]."""
    import torch
    if inv_temperature is None:
        return None
    if torch.is_tensor(inv_temperature):
        t = inv_temperature
        if t.dtype != torch.float32 or t.dim() != 1 or t.numel() != n_slots or not t.is_contiguous():
            raise ValueError(f"inv_temperature must be a contiguous float32 tensor [{n_slots}] (one beta per slot)")
        return t
    vals = [float(inv_temperature)] * n_slots if isinstance(inv_temperature, (int, float, np.floating, np.integer)) \
        else [float(v) for v in inv_temperature]
    if len(vals) != n_slots:
        raise ValueError(f"{len(vals)} inverse temperatures for {n_slots} slots")
    for v in vals:
        if not (v > 0.0 and v != float("inf")):
            raise ValueError(f"inv_temperature must be positive and finite, got {v!r}")
    return vals


def _beta_tensor(beta, device):
    import torch
    if beta is None or torch.is_tensor(beta):
        if beta is not None:
            _native.require_hip(beta)
        return beta
    return torch.tensor(beta, dtype=torch.float32, device=device)


def _slot_ce_forward(logits, labels, spec, weights, labels_b, lam, eps, want_grad):
    """Validates on the host, then one ``sir_ce_loss_slots`` launch -> (loss [], slot_loss [G], dlogits or None)."""
    import torch
    from .featurizer import get_featurizer
    _check_logits(logits, spec)
    _check_labels(labels, logits, spec)
    if lam is not None and labels_b is None:
        raise ValueError("lam weighs labels against labels_b, which was not given")
    if labels_b is not None:
        _check_labels(labels_b, logits, spec, "labels_b")
    if lam is not None and (not torch.is_tensor(lam) or lam.dtype != torch.float32 or lam.numel() != logits.shape[0]):
        raise ValueError("lam must be a float32 tensor with one value per row")
    _native.require_hip(logits, labels, labels_b, lam)
    lib = _native.lib()
    logits, labels = logits.contiguous(), labels.contiguous()
    labels_b = labels_b.contiguous() if labels_b is not None else None
    lam = lam.contiguous() if lam is not None else None
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    slot_loss = torch.empty(spec.n_slots, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits) if want_grad else None
    w = (C.c_float * spec.n_slots)(*weights) if weights is not None else None
    rc = lib.sir_ce_loss_slots(get_featurizer().handle, logits.data_ptr(), labels.data_ptr(),
                               labels_b.data_ptr() if labels_b is not None else None,
                               lam.data_ptr() if lam is not None else None, eps, _sizes_array(spec), w, spec.n_slots,
                               logits.shape[0], spec.total, loss.data_ptr(), slot_loss.data_ptr(),
                               dlogits.data_ptr() if dlogits is not None else None, 1.0, _native.current_stream_ptr())
    _native.check(rc, "sir_ce_loss_slots")
    return loss, slot_loss, dlogits


def _autograd_fn():
    """The autograd function around ``sir_ce_loss_slots`` (built on first use: torch is imported lazily, as in metrics)."""
    global _SlotCE
    if _SlotCE is None:
        import torch

        class SlotCE(torch.autograd.Function):
            @staticmethod
            def forward(ctx, logits, labels, spec, weights, labels_b, lam, eps):
                loss, slot_loss, dlogits = _slot_ce_forward(logits, labels, spec, weights, labels_b, lam, eps,
                                                            ctx.needs_input_grad[0])
                ctx.dlogits = dlogits
                ctx.mark_non_differentiable(slot_loss)
                return loss, slot_loss

            @staticmethod
            def backward(ctx, grad_out, _grad_slot):
                return ctx.dlogits * grad_out, None, None, None, None, None, None

        _SlotCE = SlotCE
    return _SlotCE


_SlotCE = None


def slot_cross_entropy(logits, labels, spec, weights=None, labels_b=None, lam=None, label_smoothing=0.0, return_slot_losses=False):
    """``sum_g w_g * CE(logits[:, segment g], labels[:, g])`` by one ``sir_ce_loss_slots`` launch, differentiable in
    ``logits``.  Per slot the loss is ``train_ops.fused_cross_entropy``'s on the segment (``label_smoothing`` eps spreads
    eps / C_g inside slot g; ``labels_b`` [B, G] and the per-row ``lam`` [B] are mixup's second labels and weight); a label
    of -100 takes its row out of that slot only.  ``return_slot_losses=True`` appends the device tensor [G] of the slots'
    un-weighted losses."""
    spec = _as_spec(spec)
    weights = check_weights(weights, spec.n_slots)
    eps = _check_smoothing(label_smoothing)
    loss, slot_loss = _autograd_fn().apply(logits, labels, spec, weights, labels_b, lam, eps)
    return (loss, slot_loss) if return_slot_losses else loss


class SlotLoss:
    """Callable criterion of ``train()`` under a slot layout: ``criterion(logits, labels [B, G], labels_b=None, lam=None)``.
    ``last_slot_losses``: the device tensor [G] of the latest call's un-weighted per-slot losses (no copy is made)."""

    def __init__(self, spec, weights=None, label_smoothing=0.0):
        self.spec = _as_spec(spec)
        self.weights = check_weights(weights, self.spec.n_slots)
        self.label_smoothing = _check_smoothing(label_smoothing)
        self.last_slot_losses = None

    def __call__(self, logits, labels, labels_b=None, lam=None):
        loss, self.last_slot_losses = slot_cross_entropy(logits, labels, self.spec, self.weights, labels_b, lam,
                                                         self.label_smoothing, return_slot_losses=True)
        return loss


def _check_k(k):
    if isinstance(k, bool) or not hasattr(k, "__index__") or not 1 <= int(k) <= 8:
        raise ValueError(f"k must be an integer in [1, 8], got {k!r}")
    return int(k)


def classify(logits, spec, k=1, inv_temperature=None, want_probs=False):
    """Segment-wise softmax and top-k in one ``sir_classify_slots`` launch -> ``(topk_idx int32 [B, G, k], topk_prob float32
    [B, G, k], joint_prob float32 [B])``: slot-local class indices by descending logit (ranks beyond a slot's width hold
    -1 / 0), and the product of the slots' top probabilities.  ``inv_temperature``: None, a number, one per slot, or a device
    tensor [G] (``fit_slot_temperatures``).  A slot whose segment holds a NaN or an infinity comes back as -1 / NaN and makes
    the row's joint NaN.  ``want_probs=True`` appends the segment-wise softmax [B, total]."""
    import torch
    from .featurizer import get_featurizer
    spec = _as_spec(spec)
    _check_logits(logits, spec)
    k = _check_k(k)
    beta = check_inv_temperature(inv_temperature, spec.n_slots)
    _native.require_hip(logits)
    lib = _native.lib()
    logits = logits.contiguous()
    beta = _beta_tensor(beta, logits.device)
    bsz, g = logits.shape[0], spec.n_slots
    idx = torch.empty((bsz, g, k), dtype=torch.int32, device=logits.device)
    prob = torch.empty((bsz, g, k), dtype=torch.float32, device=logits.device)
    joint = torch.empty((bsz,), dtype=torch.float32, device=logits.device)
    probs = torch.empty_like(logits) if want_probs else None
    rc = lib.sir_classify_slots(get_featurizer().handle, logits.data_ptr(), bsz, spec.total, _sizes_array(spec), g,
                                beta.data_ptr() if beta is not None else None, k,
                                probs.data_ptr() if probs is not None else None, idx.data_ptr(), prob.data_ptr(),
                                joint.data_ptr(), _native.current_stream_ptr())
    _native.check(rc, "sir_classify_slots")
    return (idx, prob, joint, probs) if want_probs else (idx, prob, joint)


# ---- joint decoding -----------------------------------------------------------------------------------------------------------
MAX_TUPLES = 4096
TUPLE_BYTES = 8


def pack_tuples(rows, n_slots):
    """Label tuples [N, G] -> the table ``sir_decode_slots`` reads: uint8 numpy [N, 8], byte g the slot-local label of slot g,
    bytes g >= n_slots zero."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, n_slots)
    packed = np.zeros((rows.shape[0], TUPLE_BYTES), dtype=np.uint8)
    packed[:, :n_slots] = rows
    return packed


class TupleTable:
    """The label tuples that exist: what constrained decoding (``decode(..., table=)``) ranks.  Row t of the table is the tuple
    ``rows[t]`` of slot-local labels; a tie between equal scores goes to the lower row.  Validated on the host: 1 .. 4096 rows,
    every label inside its slot, no tuple twice."""

    def __init__(self, spec, rows):
        self.spec = _as_spec(spec)
        g = self.spec.n_slots
        try:
            rows = [tuple(r) for r in rows]
        except TypeError:
            raise ValueError("a tuple table needs a sequence of label tuples") from None
        if not 1 <= len(rows) <= MAX_TUPLES:
            raise ValueError(f"a tuple table has 1..{MAX_TUPLES} rows, got {len(rows)}")
        index = {}
        for t, r in enumerate(rows):
            if len(r) != g:
                raise ValueError(f"row {t} has {len(r)} labels for {g} slots")
            for v, c in zip(r, self.spec.sizes):
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < c:
                    raise ValueError(f"row {t}: label {v!r} outside its slot's [0, {c})")
            r = tuple(int(v) for v in r)
            if r in index:
                raise ValueError(f"rows {index[r]} and {t} hold the same tuple {r}")
            index[r] = t
        self.rows = tuple(index)                      # (insertion order = row order)
        self.index = index
        self.packed = pack_tuples(self.rows, g)
        self._device = {}

    def __len__(self):
        return len(self.rows)

    def __eq__(self, other):
        return isinstance(other, TupleTable) and self.spec == other.spec and self.rows == other.rows

    @classmethod
    def full(cls, spec):
        """Every tuple of the product space, in lexicographic order (slot 0 most significant): row t is the tuple whose
        mixed-radix number is t, unconstrained decoding's ``best_index``.  Refused above 4096 tuples."""
        import itertools
        spec = _as_spec(spec)
        n = int(np.prod([int(c) for c in spec.sizes], dtype=object))
        if n > MAX_TUPLES:
            raise ValueError(f"the layout {spec.sizes} has {n} tuples, a table holds at most {MAX_TUPLES}")
        return cls(spec, itertools.product(*[range(c) for c in spec.sizes]))

    @classmethod
    def from_dataframe(cls, spec, dataframe):
        """The distinct tuples the data contains, sorted.  A row with a value outside the spec's vocabularies names no tuple
        and is left out."""
        spec = _as_spec(spec)
        labels = spec.encode(dataframe)
        known = labels[(labels != IGNORE).all(axis=1)]
        return cls(spec, sorted({tuple(int(v) for v in r) for r in known}))

    @classmethod
    def from_csv(cls, spec, csv):
        import pandas as pd
        return cls.from_dataframe(spec, pd.read_csv(csv))

    def to_dict(self):
        return {"columns": list(self.spec.columns), "vocab": {c: list(vs) for c, vs in zip(self.spec.columns, self.spec.vocab)},
                "tuples": [list(r) for r in self.rows]}

    def save(self, path):
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=2)

    @classmethod
    def load(cls, path, spec=None):
        """The table of ``save``; with ``spec`` given, the file's layout must be that spec's."""
        with open(path, "r") as f:
            d = json.load(f)
        if not isinstance(d, dict) or not {"columns", "vocab", "tuples"} <= set(d):
            raise ValueError(f"{path}: not a tuple table (needs 'columns', 'vocab' and 'tuples')")
        own = SlotSpec(d["columns"], d["vocab"])
        if spec is not None and own != _as_spec(spec):
            raise ValueError(f"{path}: the table's slot layout is not the given one")
        return cls(own if spec is None else spec, d["tuples"])

    def encode(self, labels):
        """Slot labels [N, G] (numpy or tensor) -> int64 numpy [N]: the table row of each label tuple, -100 for a tuple that is not
        in the table or has a -100 slot."""
        if hasattr(labels, "detach"):
            labels = labels.detach().cpu().numpy()
        labels = np.asarray(labels, dtype=np.int64)
        if labels.ndim != 2 or labels.shape[1] != self.spec.n_slots:
            raise ValueError(f"labels must be [N, {self.spec.n_slots}] (one column per slot), got {labels.shape}")
        return np.asarray([self.index.get(tuple(r), IGNORE) for r in labels.tolist()], dtype=np.int64).reshape(-1)

    def names(self):
        """One name per row: the reference's ``action_object`` join where that is unique over the table, else all values joined
        by ``_``."""
        decoded = [self.spec.decode(r) for r in self.rows]
        short = [self.spec.reference_label(d) for d in decoded]
        if None not in short and len(set(short)) == len(short):
            return short
        return ["_".join(d[c] for c in self.spec.columns) for d in decoded]

    def device_tensor(self, device):
        """The packed table on ``device`` (uint8 [N, 8], uploaded once per device)."""
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.packed).to(device)
        return self._device[key]


def decode(logits, spec, table=None, k=1, inv_temperature=None, want_mass=False, want_scores=False):
    """The k best label tuples of every row in one ``sir_decode_slots`` launch -> ``(best_index int32 [B, k], best_labels int32
    [B, k, G], best_logp float32 [B, k], best_prob float32 [B, k])``, then ``valid_mass`` [B] with ``want_mass`` and
    ``tuple_logp`` [B, len(table)] with ``want_scores`` (which needs a table).

    With ``table`` (a ``TupleTable``) only its tuples are ranked, ``best_index`` is the table row and ``best_prob`` the
    softmax over the table of the tuples' summed log-probabilities; ``valid_mass`` is the probability the independent heads
    put on the table.  Without one the whole product space is ranked, ``best_index`` is the tuple's mixed-radix number and
    ``best_prob`` the product of the slots' probabilities.  Ranks that do not exist hold -1 / -1 / -inf / 0; a row with a NaN
    or an infinity in any segment comes back as -1 / NaN."""
    import torch
    from .featurizer import get_featurizer
    spec = _as_spec(spec)
    _check_logits(logits, spec)
    k = _check_k(k)
    beta = check_inv_temperature(inv_temperature, spec.n_slots)
    if table is not None:
        if not isinstance(table, TupleTable):
            raise ValueError("table must be a slots.TupleTable")
        if table.spec.sizes != spec.sizes:
            raise ValueError(f"the table was built for the layout {table.spec.sizes}, the logits are read as {spec.sizes}")
    elif want_scores:
        raise ValueError("want_scores returns one score per table row: it needs a table")
    _native.require_hip(logits)
    lib = _native.lib()
    logits = logits.contiguous()
    beta = _beta_tensor(beta, logits.device)
    bsz, g, dev = logits.shape[0], spec.n_slots, logits.device
    tuples = table.device_tensor(dev) if table is not None else None
    n = len(table) if table is not None else 0
    index = torch.empty((bsz, k), dtype=torch.int32, device=dev)
    labels = torch.empty((bsz, k, g), dtype=torch.int32, device=dev)
    logp = torch.empty((bsz, k), dtype=torch.float32, device=dev)
    prob = torch.empty((bsz, k), dtype=torch.float32, device=dev)
    mass = torch.empty((bsz,), dtype=torch.float32, device=dev) if want_mass else None
    scores = torch.empty((bsz, n), dtype=torch.float32, device=dev) if want_scores else None
    rc = lib.sir_decode_slots(get_featurizer().handle, logits.data_ptr(), bsz, spec.total, _sizes_array(spec), g,
                              beta.data_ptr() if beta is not None else None, tuples.data_ptr() if tuples is not None else None, n, k,
                              index.data_ptr(), labels.data_ptr(), logp.data_ptr(), prob.data_ptr(),
                              mass.data_ptr() if mass is not None else None, scores.data_ptr() if scores is not None else None,
                              _native.current_stream_ptr())
    _native.check(rc, "sir_decode_slots")
    out = (index, labels, logp, prob)
    if want_mass:
        out += (mass,)
    if want_scores:
        out += (scores,)
    return out


class ConstrainedEvalAccumulator:
    """Evaluation under constrained decoding, kept on the device: per batch one ``sir_decode_slots`` launch over ``table``
    (k = 1, ``valid_mass``, and ``tuple_logp`` for a table of at most 64 rows).  Exact match is counted against
    ``table.encode(labels)``; for a table of at most 64 rows ``tuple_logp`` and those encoded labels also go to an unchanged
    ``metrics.EvalAccumulator`` -- the softmax of the tuple scores IS the posterior over the table -- which gives the
    classification report over the intents and NLL / ECE / MCE of that posterior.  A clip whose tuple is not in the table (or has a
    -100 slot) is left out of the counts, as a -100 label is elsewhere."""

    def __init__(self, spec, table, n_bins=15, inv_temperature=None):
        self.spec = _as_spec(spec)
        if not isinstance(table, TupleTable) or table.spec.sizes != self.spec.sizes:
            raise ValueError("table must be a slots.TupleTable of the same slot layout")
        self.table = table
        self.n_bins = int(n_bins)
        self._inv_temperature = check_inv_temperature(inv_temperature, self.spec.n_slots)
        self.posterior = metrics.EvalAccumulator(len(table), n_bins) if len(table) <= MAX_CLASSES else None
        self._counts = None                  # device int64 {n, exact_match, rows with a finite mass}
        self._mass = None                    # device float64 {sum of valid_mass}

    def update(self, logits, labels):
        """Add one batch: logits float32 [B, total] on the device; labels int64 [B, G], on the HOST (they are encoded there, before
        anything is queued) or on the device (copied back first).  Nothing else comes back."""
        import torch
        y = torch.from_numpy(self.table.encode(labels)).to(logits.device, non_blocking=True)
        if self._counts is None:
            self._counts = torch.zeros(3, dtype=torch.int64, device=logits.device)
            self._mass = torch.zeros(1, dtype=torch.float64, device=logits.device)
        out = decode(logits, self.spec, table=self.table, k=1, inv_temperature=self._inv_temperature, want_mass=True,
                     want_scores=self.posterior is not None)
        best, mass = out[0][:, 0].to(torch.int64), out[4]
        counted = (y != IGNORE) & (best >= 0)
        finite = torch.isfinite(mass)
        self._counts += torch.stack([counted.sum(), (counted & (best == y)).sum(), finite.sum()])
        self._mass += torch.where(finite, mass, torch.zeros_like(mass)).double().sum()
        if self.posterior is not None:
            self.posterior.update(out[5], y)
        return self

    def state_arrays(self):
        counts = np.zeros(3, dtype=np.int64) if self._counts is None else self._counts.cpu().numpy()
        mass = 0.0 if self._mass is None else float(self._mass.cpu().numpy()[0])
        out = {"n": int(counts[0]), "exact_match": int(counts[1]), "mass_rows": int(counts[2]), "mass_sum": mass}
        if self.posterior is not None:
            out["posterior"] = self.posterior.state_arrays()
        return out


def merge_constrained(a, b):
    out = {k: a[k] + b[k] for k in ("n", "exact_match", "mass_rows", "mass_sum")}
    if "posterior" in a:
        out["posterior"] = metrics.merge(a["posterior"], b["posterior"])
    return out


def constrained_json(arrays, table):
    """``constrained_metrics.json`` of scripts/evaluate.py from ``ConstrainedEvalAccumulator.state_arrays()`` -> (dict, the
    classification report's text or None)."""
    nan = float("nan")
    n = arrays["n"]
    out = {"n": n, "n_tuples": len(table), "exact_match": arrays["exact_match"],
           "exact_match_accuracy": arrays["exact_match"] / n if n else nan,
           "mean_valid_mass": arrays["mass_sum"] / arrays["mass_rows"] if arrays["mass_rows"] else nan}
    text = None
    if "posterior" in arrays:
        report = metrics.report_from_state(arrays["posterior"], table.names())
        calib = metrics.calibration_json(report)
        out.update({k: calib[k] for k in ("nll", "ece", "mce") if k in calib})
        out["calibration"] = calib
        text = metrics.format_report(report["classification"])
    return out, text


# ---- evaluation state ---------------------------------------------------------------------------------------------------------
def joint_field_words(n_bins):
    """8-byte words of the joint block's fields: n, exact_match, slots_correct [9], nll_sum, three bin tables, n_excluded."""
    metrics._check_sizes(1, n_bins)
    return 2 + JOINT_SLOTS_CORRECT + 1 + 3 * n_bins + 1


def joint_words(n_bins):
    return joint_field_words(n_bins) + metrics.SCRATCH_BLOCKS * (n_bins + 1)


def state_words(sizes, n_bins):
    """8-byte words of the device state (``sir_eval_slots_state_bytes`` / 8): the slots' single-head states back to back, then
    the joint block."""
    sizes = check_sizes(sizes)
    return sum(metrics.state_words(c, n_bins) for c in sizes) + joint_words(n_bins)


def unpack_joint(words, n_bins):
    words = np.ascontiguousarray(np.asarray(words, dtype=np.int64))
    if words.shape != (joint_words(n_bins),):
        raise ValueError(f"joint block of {words.shape} words, expected ({joint_words(n_bins)},)")
    m, o = n_bins, 2 + JOINT_SLOTS_CORRECT
    out = {"n": int(words[0]), "exact_match": int(words[1]), "slots_correct": words[2: o].copy(),
           "nll_sum": float(words[o: o + 1].view(np.float64)[0])}
    o += 1
    out.update(metrics.unpack_bins(words, o, m))
    out["n_excluded"] = int(words[o + 3 * m])
    return out


def unpack_state(words, sizes, n_bins):
    """The raw state -> ``{"slots": [single-head dicts, as metrics.unpack_state], "joint": dict}``."""
    sizes = check_sizes(sizes)
    words = np.ascontiguousarray(np.asarray(words, dtype=np.int64))
    if words.shape != (state_words(sizes, n_bins),):
        raise ValueError(f"state of {words.shape} words, expected ({state_words(sizes, n_bins)},)")
    slots, o = [], 0
    for c in sizes:
        n = metrics.state_words(c, n_bins)
        slots.append(metrics.unpack_state(words[o: o + n], c, n_bins))
        o += n
    return {"slots": slots, "joint": unpack_joint(words[o:], n_bins)}


def merge(a, b):
    """The state of the rows of ``a`` and ``b`` together (per-rank shards): every field adds."""
    if len(a["slots"]) != len(b["slots"]) or len(a["joint"]["bin_count"]) != len(b["joint"]["bin_count"]):
        raise ValueError("states of different slot layouts or n_bins cannot be merged")
    joint = metrics.add_fields(a["joint"], b["joint"], _JOINT_INT_FIELDS, _JOINT_FLOAT_FIELDS)
    return {"slots": [metrics.merge(x, y) for x, y in zip(a["slots"], b["slots"])], "joint": joint}


def joint_report(joint):
    """``{n, exact_match_accuracy, nll, ece, mce, slots_correct, n_excluded}`` (+ ``reliability``) from the joint block, in
    float64; ECE / MCE are those of ``metrics.report_from_state`` with the joint confidence and exact match as "correct"."""
    n = int(joint["n"])
    if int(np.asarray(joint["bin_count"], dtype=np.int64).sum()) != n or int(np.asarray(joint["slots_correct"]).sum()) != n:
        raise ValueError("inconsistent joint block: the bins or slots_correct do not add up to n")
    nan = float("nan")
    ece, mce, reliability = metrics.calibration_from_bins(joint["bin_count"], joint["bin_correct"], joint["bin_conf_sum"], n)
    return {"n": n, "n_excluded": int(joint["n_excluded"]),
            "exact_match_accuracy": int(joint["exact_match"]) / n if n else nan,
            "nll": float(joint["nll_sum"]) / n if n else nan,
            "ece": ece, "mce": mce,
            "slots_correct": np.asarray(joint["slots_correct"], dtype=np.int64),
            "reliability": reliability}


def joint_json(report):
    """The JSON-serialisable form of ``joint_report``'s result (``joint_metrics.json`` of scripts/evaluate.py)."""
    out = {k: report[k] for k in ("n", "n_excluded", "exact_match_accuracy", "nll", "ece", "mce")}
    out["slots_correct"] = metrics.json_list(report["slots_correct"])
    out["reliability"] = {k: metrics.json_list(v) for k, v in report["reliability"].items()}
    return out


class SlotEvalAccumulator(metrics.DeviceState):
    """``metrics.EvalAccumulator`` under a slot layout: one device buffer holding a single-head state per slot and the joint
    block, filled by ``sir_eval_accumulate_slots`` batch by batch with no copy and no synchronisation."""
    _layout_error = "sir_eval_slots_state_bytes disagrees with the layout of sir_amd.slots"
    _beta_tensor = staticmethod(_beta_tensor)

    def __init__(self, spec, n_bins=15, inv_temperature=None):
        self.spec = _as_spec(spec)
        metrics._check_sizes(1, n_bins)
        self.n_bins = int(n_bins)
        self._inv_temperature = check_inv_temperature(inv_temperature, self.spec.n_slots)
        self._merged = None

    def _library_bytes(self):
        return _native.lib().sir_eval_slots_state_bytes(_sizes_array(self.spec), self.spec.n_slots, self.n_bins)

    def _layout_words(self):
        return state_words(self.spec.sizes, self.n_bins)

    def update(self, logits, labels):
        """Add one batch: logits float32 [B, total], labels int64 [B, G], both on the device.  Nothing comes back."""
        from .featurizer import get_featurizer
        _check_logits(logits, self.spec)
        _check_labels(labels, logits, self.spec)
        _native.require_hip(logits, labels)
        self._ensure(logits.device)
        logits, labels = logits.contiguous(), labels.contiguous()
        rc = _native.lib().sir_eval_accumulate_slots(get_featurizer().handle, logits.data_ptr(), labels.data_ptr(), logits.shape[0],
                                                     self.spec.total, _sizes_array(self.spec), self.spec.n_slots,
                                                     self._beta.data_ptr() if self._beta is not None else None, self.n_bins,
                                                     self._state.data_ptr(), self._state.numel() * 8, _native.current_stream_ptr())
        _native.check(rc, "sir_eval_accumulate_slots")
        return self

    def reset(self):
        self._merged = None
        return super().reset()

    def merge(self, arrays):
        """Add another shard's ``state_arrays()`` (data-parallel evaluation: gather the ranks' states, merge on one)."""
        self._merged = arrays if self._merged is None else merge(self._merged, arrays)
        return self

    def state_arrays(self):
        """``{"slots": [...], "joint": {...}}`` as numpy -- the one device-to-host copy -- plus whatever was merged in."""
        own = unpack_state(self._words(), self.spec.sizes, self.n_bins)
        return own if self._merged is None else merge(own, self._merged)

    def result(self, target_names=None):
        """``{"slots": {column: metrics.report_from_state(...)}, "joint": joint_report(...)}``.  ``target_names``: None (the
        spec's vocabularies) or a dict column -> names."""
        arrays = self.state_arrays()
        names = {c: list(vs) for c, vs in zip(self.spec.columns, self.spec.vocab)}
        if target_names is not None:
            names.update(target_names)
        return {"slots": {c: metrics.report_from_state(a, names[c]) for c, a in zip(self.spec.columns, arrays["slots"])},
                "joint": joint_report(arrays["joint"])}


def fit_slot_temperatures(logits, labels, spec, iters=20):
    """``metrics.fit_temperature`` on each segment's contiguous copy -> float32 device tensor [G] of the fitted betas, a valid
    ``inv_temperature`` of ``classify`` and ``SlotEvalAccumulator``.  No new kernel; nothing is copied to the host."""
    import torch
    spec = _as_spec(spec)
    _check_logits(logits, spec)
    _check_labels(labels, logits, spec)
    if not (isinstance(iters, (int, np.integer)) and 0 <= iters <= 1000):
        raise ValueError(f"iters must be an integer in [0, 1000], got {iters!r}")
    _native.require_hip(logits, labels)
    betas = [metrics.fit_temperature(logits[:, s: s + c].contiguous(), labels[:, g].contiguous(), iters)[:1]
             for g, (s, c) in enumerate(zip(spec.starts, spec.sizes))]
    return torch.cat(betas)
