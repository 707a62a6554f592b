"""Evaluation on the device: what ``scripts/evaluate.py`` used to hand to sklearn, plus calibration.

``EvalAccumulator`` owns one small device buffer (``sir_eval_state_bytes``) and adds every batch of logits and labels
into it with one ``sir_eval_accumulate`` launch: no per-batch copy, no synchronisation.  ``state_arrays()`` is the one
device-to-host copy; everything after it (``report_from_state``, ``merge``, ``format_report``) is host code in float64
on a few kilobytes.  ``fit_temperature`` is temperature scaling (Guo et al. 2017, "On Calibration of Modern Neural
Networks") by ``sir_temperature_fit``: the fitted ``beta = 1 / T`` stays on the device and can be handed to
``EvalAccumulator``, ``ops.classify`` and ``CNNAudioGRU.classify`` as ``inv_temperature``.

State layout (include/sir_hip.h), every field 8 bytes: confusion [C][C], n, topk_correct [8], nll_sum (double),
bin_count [M], bin_correct [M], bin_conf_sum [M] (double), n_ignored, n_nonfinite, then the kernels' scratch area.
"""
import numpy as np

MAX_CLASSES = 64
MAX_BINS = 64
TOPK_SLOTS = 8
SCRATCH_BLOCKS = 64          # the kernels' own partial sums behind the fields: [SCRATCH_BLOCKS][n_bins + 1] doubles
_INT_FIELDS = ("confusion", "n", "topk_correct", "bin_count", "bin_correct", "n_ignored", "n_nonfinite")
_FLOAT_FIELDS = ("nll_sum", "bin_conf_sum")


def _check_sizes(num_classes, n_bins):
    if not (isinstance(num_classes, (int, np.integer)) and 1 <= num_classes <= MAX_CLASSES):
        raise ValueError(f"num_classes must be an integer in [1, {MAX_CLASSES}], got {num_classes!r}")
    if not (isinstance(n_bins, (int, np.integer)) and 1 <= n_bins <= MAX_BINS):
        raise ValueError(f"n_bins must be an integer in [1, {MAX_BINS}], got {n_bins!r}")


def field_words(num_classes, n_bins):
    """8-byte words of the fields of the device state (what ``unpack_state`` reads)."""
    _check_sizes(num_classes, n_bins)
    return num_classes * num_classes + 1 + TOPK_SLOTS + 1 + 3 * n_bins + 2


def state_words(num_classes, n_bins):
    """8-byte words of the device state (``sir_eval_state_bytes`` / 8): the fields, then the kernels' scratch area."""
    return field_words(num_classes, n_bins) + SCRATCH_BLOCKS * (n_bins + 1)


def unpack_state(words, num_classes, n_bins):
    """The raw state (int64 array of ``state_words`` entries, doubles still as bit patterns) -> dict of arrays (the scratch
    area behind the fields is not looked at)."""
    words = np.ascontiguousarray(np.asarray(words, dtype=np.int64))
    if words.shape != (state_words(num_classes, n_bins),):
        raise ValueError(f"state of {words.shape} words, expected ({state_words(num_classes, n_bins)},)")
    c, m = num_classes, n_bins
    o = c * c
    out = {"confusion": words[:o].reshape(c, c).copy(), "n": int(words[o]), "topk_correct": words[o + 1: o + 9].copy(),
           "nll_sum": float(words[o + 9: o + 10].view(np.float64)[0])}
    o += 10
    out.update(unpack_bins(words, o, m))
    out["n_ignored"] = int(words[o + 3 * m])
    out["n_nonfinite"] = int(words[o + 3 * m + 1])
    return out


def unpack_bins(words, o, n_bins):
    """The three bin tables that start at word ``o`` of a raw state (here and in ``slots.unpack_joint``): ``bin_count`` and
    ``bin_correct`` int64, ``bin_conf_sum`` the doubles behind their bit patterns."""
    m = n_bins
    return {"bin_count": words[o: o + m].copy(), "bin_correct": words[o + m: o + 2 * m].copy(),
            "bin_conf_sum": words[o + 2 * m: o + 3 * m].view(np.float64).copy()}


def _check_state(a):
    missing = [k for k in _INT_FIELDS + _FLOAT_FIELDS if k not in a]
    if missing:
        raise ValueError(f"state is missing {missing}")
    cm = np.asarray(a["confusion"])
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1] or not 1 <= cm.shape[0] <= MAX_CLASSES:
        raise ValueError(f"confusion must be [C][C] with C in [1, {MAX_CLASSES}], got {cm.shape}")
    m = np.asarray(a["bin_count"]).shape
    if len(m) != 1 or not 1 <= m[0] <= MAX_BINS or np.asarray(a["bin_correct"]).shape != m or np.asarray(a["bin_conf_sum"]).shape != m:
        raise ValueError("bin_count, bin_correct and bin_conf_sum must be one-dimensional and of one length in [1, 64]")
    if np.asarray(a["topk_correct"]).shape != (TOPK_SLOTS,):
        raise ValueError(f"topk_correct must hold {TOPK_SLOTS} entries")


def merge(a, b):
    """The state of the rows of ``a`` and ``b`` together (per-rank shards, per-split shards): every field adds."""
    _check_state(a)
    _check_state(b)
    if np.asarray(a["confusion"]).shape != np.asarray(b["confusion"]).shape or len(a["bin_count"]) != len(b["bin_count"]):
        raise ValueError("states of different num_classes or n_bins cannot be merged")
    return add_fields(a, b, _INT_FIELDS, _FLOAT_FIELDS)


def add_fields(a, b, int_fields, float_fields):
    """``{field: a[field] + b[field]}``, the int fields first (``merge`` here, the joint block of ``slots.merge``): scalars
    come back as Python ``int`` / ``float``, arrays as ``int64`` / ``float64``."""
    out = {}
    for fields, dtype, scalar in ((int_fields, np.int64, int), (float_fields, np.float64, float)):
        for k in fields:
            s = np.asarray(a[k], dtype=dtype) + np.asarray(b[k], dtype=dtype)
            out[k] = scalar(s) if s.ndim == 0 else s
    return out


def _prf(tp, pred_sum, true_sum):
    """precision, recall, F1 with sklearn's ``zero_division=0`` (0 where the denominator is 0)."""
    tp, pred_sum, true_sum = (np.asarray(v, dtype=np.float64) for v in (tp, pred_sum, true_sum))
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(pred_sum > 0, tp / pred_sum, 0.0)
        r = np.where(true_sum > 0, tp / true_sum, 0.0)
        f = np.where(p + r > 0, 2 * p * r / (p + r), 0.0)
    return p, r, f


def _average(p, r, f, support, weights):
    if weights is None:
        return float(np.mean(p)), float(np.mean(r)), float(np.mean(f))
    if weights.sum() == 0:
        return 0.0, 0.0, 0.0
    return tuple(float(np.average(v, weights=weights)) for v in (p, r, f))


def classification_from_confusion(confusion, target_names=None, labels=None):
    """sklearn's ``classification_report(y_true, y_pred, labels=labels, target_names=target_names, output_dict=True,
    zero_division=0)`` computed from the confusion matrix alone (row = true label, column = prediction).
    ``labels`` (default: every class) restricts the rows of the report as sklearn's ``labels=`` does; when a label that
    occurs (as truth or prediction) is left out, the ``accuracy`` entry becomes ``micro avg``, as there."""
    cm = np.asarray(confusion, dtype=np.int64)
    c = cm.shape[0]
    labels = list(range(c)) if labels is None else [int(v) for v in labels]
    if any(not 0 <= v < c for v in labels):
        raise ValueError(f"labels must lie in [0, {c})")
    names = [str(v) for v in labels] if target_names is None else [str(v) for v in target_names]
    if len(names) != len(labels):
        raise ValueError(f"{len(names)} target_names for {len(labels)} labels")
    tp_all, pred_all, true_all = np.diag(cm), cm.sum(0), cm.sum(1)
    idx = np.asarray(labels, dtype=np.int64)
    tp, pred_sum, true_sum = tp_all[idx], pred_all[idx], true_all[idx]
    p, r, f = _prf(tp, pred_sum, true_sum)
    report = {name: {"precision": float(p[i]), "recall": float(r[i]), "f1-score": float(f[i]), "support": int(true_sum[i])}
              for i, name in enumerate(names)}
    present = {int(i) for i in np.nonzero((pred_all > 0) | (true_all > 0))[0]}
    total = int(true_sum.sum())
    mp, mr, mf = _prf(tp.sum(), pred_sum.sum(), true_sum.sum())
    if present <= set(labels):
        report["accuracy"] = float(mp)            # micro precision = recall = F1 = accuracy when no label is left out
    else:
        report["micro avg"] = {"precision": float(mp), "recall": float(mr), "f1-score": float(mf), "support": total}
    for name, w in (("macro avg", None), ("weighted avg", true_sum.astype(np.float64))):
        ap, ar, af = _average(p, r, f, true_sum, w)
        report[name] = {"precision": ap, "recall": ar, "f1-score": af, "support": total}
    return report


def format_report(report, digits=2):
    """The text sklearn's ``classification_report`` (``output_dict=False``) prints for ``report``, a dict as
    ``classification_from_confusion`` / sklearn's ``output_dict=True`` return it.  (One difference: when not a single prediction
    is correct, sklearn 1.7 prints the supports as floats, ``6.0``; here they are integers always.)"""
    tail = [k for k in ("accuracy", "micro avg", "macro avg", "weighted avg") if k in report]
    names = [k for k in report if k not in tail]
    width = max([len(n) for n in names] + [len("weighted avg"), digits])
    headers = ["precision", "recall", "f1-score", "support"]
    text = "{:>{width}s} ".format("", width=width) + "".join(" {:>9}".format(v) for v in headers) + "\n\n"
    row_fmt = "{:>{width}s} " + " {:>9.{digits}f}" * 3 + " {:>9}\n"
    for n in names:
        e = report[n]
        text += row_fmt.format(n, e["precision"], e["recall"], e["f1-score"], e["support"], width=width, digits=digits)
    text += "\n"
    support = report["weighted avg"]["support"]
    for n in tail:
        if n == "accuracy":
            text += ("{:>{width}s} " + " {:>9.{digits}}" * 2 + " {:>9.{digits}f}" + " {:>9}\n").format(
                n, "", "", report[n], support, width=width, digits=digits)
        else:
            e = report[n]
            text += row_fmt.format(n, e["precision"], e["recall"], e["f1-score"], e["support"], width=width, digits=digits)
    return text


def report_from_state(arrays, target_names=None):
    """Everything the evaluation reports, from one state (``EvalAccumulator.state_arrays()``, ``merge``), in float64:

    ``n``, ``n_ignored``, ``n_nonfinite``, ``accuracy``, ``top1`` / ``top3`` / ``top5`` (and ``topk_accuracy`` [8]), ``nll`` (mean),
    ``confusion``, ``classification`` (per-class precision / recall / F1 / support with macro and weighted averages:
    sklearn's ``classification_report(output_dict=True, zero_division=0)`` layout and values), ``ece`` (expected
    calibration error, sum_m (n_m / n) |acc_m - conf_m|; Naeini et al. 2015), ``mce`` (the maximum of |acc_m - conf_m| over
    the occupied bins) and ``reliability``: per bin ``lo``, ``hi``, ``count``, ``accuracy``, ``confidence`` (NaN in empty bins).
    With no rows counted the rates are NaN."""
    _check_state(arrays)
    cm = np.asarray(arrays["confusion"], dtype=np.int64)
    n = int(arrays["n"])
    if int(cm.sum()) != n:
        raise ValueError(f"inconsistent state: the confusion matrix holds {int(cm.sum())} rows, n = {n}")
    nan = float("nan")
    ece, mce, reliability = calibration_from_bins(arrays["bin_count"], arrays["bin_correct"], arrays["bin_conf_sum"], n)
    topk = np.asarray(arrays["topk_correct"], dtype=np.float64)
    out = {"n": n, "n_ignored": int(arrays["n_ignored"]), "n_nonfinite": int(arrays["n_nonfinite"]), "confusion": cm,
           "accuracy": float(np.trace(cm)) / n if n else nan,
           "topk_accuracy": topk / n if n else np.full(TOPK_SLOTS, nan),
           "nll": float(arrays["nll_sum"]) / n if n else nan,
           "classification": classification_from_confusion(cm, target_names),
           "ece": ece, "mce": mce, "reliability": reliability}
    for k in (1, 3, 5):
        out[f"top{k}"] = float(out["topk_accuracy"][k - 1])
    return out


def calibration_from_bins(bin_count, bin_correct, bin_conf_sum, n):
    """The bin tables of a state of ``n`` rows -> ``(ece, mce, reliability)`` in float64, for ``report_from_state`` and
    ``slots.joint_report``: per-bin accuracy and confidence are NaN in empty bins, ``ece`` is NaN with no rows counted and
    ``mce`` with no occupied bin."""
    count = np.asarray(bin_count, dtype=np.int64)
    correct = np.asarray(bin_correct, dtype=np.float64)
    conf_sum = np.asarray(bin_conf_sum, dtype=np.float64)
    m = len(count)
    nan = float("nan")
    occupied = count > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        acc_m = np.where(occupied, correct / count, nan)
        conf_m = np.where(occupied, conf_sum / count, nan)
    gap = np.abs(acc_m - conf_m)
    return (float(np.sum(np.where(occupied, count * gap, 0.0)) / n) if n else nan,
            float(np.max(gap[occupied])) if occupied.any() else nan,
            {"lo": np.arange(m) / m, "hi": (np.arange(m) + 1) / m, "count": count, "accuracy": acc_m, "confidence": conf_m})


def json_list(v):
    """An array as a JSON-serialisable list, NaN as None."""
    return [None if (isinstance(x, float) and x != x) else x for x in np.asarray(v).tolist()]


def calibration_json(report):
    """The JSON-serialisable calibration part of ``report_from_state``'s result (``calibration.json`` of evaluate.py)."""
    rel = report["reliability"]
    return {"n": report["n"], "n_ignored": report["n_ignored"], "n_nonfinite": report["n_nonfinite"],
            "accuracy": report["accuracy"], "top1": report["top1"], "top3": report["top3"], "top5": report["top5"],
            "nll": report["nll"], "ece": report["ece"], "mce": report["mce"],
            "reliability": {k: json_list(rel[k]) for k in ("lo", "hi", "count", "accuracy", "confidence")}}


def _inv_temperature_tensor(inv_temperature, device):
    """None, a positive number or a one-element float32 device tensor -> None or that tensor (never copied back)."""
    import torch
    from . import _native
    if inv_temperature is None:
        return None
    if torch.is_tensor(inv_temperature):
        t = inv_temperature
        if t.numel() < 1 or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise _native.SirError("inv_temperature must be a contiguous float32 tensor on the HIP device (its first element is read)")
        return t
    v = float(inv_temperature)
    if not (v > 0.0 and v != float("inf")):
        raise _native.SirError(f"inv_temperature must be a positive finite number, got {inv_temperature!r}")
    return torch.full((1,), v, dtype=torch.float32, device=device)


def _logits_labels(logits, labels):
    import torch
    from . import _native
    _native.require_hip(logits, labels)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise _native.SirError(f"logits must be float32 [rows, classes], got {tuple(logits.shape)} {logits.dtype}")
    if not 1 <= logits.shape[1] <= MAX_CLASSES or logits.shape[0] < 1:
        raise _native.SirError(f"logits must hold at least one row of 1..{MAX_CLASSES} classes, got {tuple(logits.shape)}")
    if labels.dim() != 1 or labels.shape[0] != logits.shape[0] or labels.dtype != torch.int64:
        raise _native.SirError(f"labels must be int64 [rows], got {tuple(labels.shape)} {labels.dtype}")
    return logits.contiguous(), labels.contiguous()


class DeviceState:
    """The device buffer of ``EvalAccumulator`` and ``slots.SlotEvalAccumulator``: int64 words, all zero until the first update.
    The accumulator says how many bytes the library wants (``_library_bytes``), how many words its Python layout has
    (``_layout_words``), what to raise when the two disagree (``_layout_error``) and how its ``_inv_temperature`` becomes a
    device tensor (``_beta_tensor``)."""
    _state = None
    _beta = None

    def _ensure(self, device):
        import torch
        from . import _native
        if self._state is None:
            nbytes = self._library_bytes()
            if nbytes != 8 * self._layout_words():
                raise _native.SirError(self._layout_error)
            self._state = torch.zeros(nbytes // 8, dtype=torch.int64, device=device)
            self._beta = self._beta_tensor(self._inv_temperature, device)
        elif self._state.device != device:
            raise _native.SirError(f"this accumulator lives on {self._state.device}, the batch on {device}")

    def reset(self):
        if self._state is not None:
            self._state.zero_()
        return self

    def _words(self):
        """The raw state on the host -- the one device-to-host copy (it waits for the updates queued so far)."""
        if self._state is None:
            return np.zeros(self._layout_words(), dtype=np.int64)
        return self._state.cpu().numpy()


class EvalAccumulator(DeviceState):
    """Counts and sums of an evaluation, kept on the device.

    ``inv_temperature``: None, a positive number or a device scalar (``fit_temperature``'s result) applied to the logits
    before the softmax; the predictions do not depend on it, the confidences and the NLL do."""
    _layout_error = "sir_eval_state_bytes disagrees with the layout of sir_amd.metrics"
    _beta_tensor = staticmethod(_inv_temperature_tensor)

    def __init__(self, num_classes, n_bins=15, inv_temperature=None):
        _check_sizes(num_classes, n_bins)
        if inv_temperature is not None and not hasattr(inv_temperature, "data_ptr"):
            v = float(inv_temperature)
            if not (v > 0.0 and v != float("inf")):
                raise ValueError(f"inv_temperature must be a positive finite number, got {inv_temperature!r}")
        self.num_classes = int(num_classes)
        self.n_bins = int(n_bins)
        self._inv_temperature = inv_temperature

    def _library_bytes(self):
        from . import _native
        return _native.lib().sir_eval_state_bytes(self.num_classes, self.n_bins)

    def _layout_words(self):
        return state_words(self.num_classes, self.n_bins)

    def update(self, logits, labels):
        """Add one batch: logits float32 [B, num_classes], labels int64 [B], both on the device.  One launch on the
        current stream, nothing comes back.  Labels of -100 are ignored; any other label outside the classes is left out
        and makes the next ``ops.check_status()`` raise; rows with a NaN or an infinity count in ``n_nonfinite`` only."""
        from . import _native
        from .featurizer import get_featurizer
        logits, labels = _logits_labels(logits, labels)
        if logits.shape[1] != self.num_classes:
            raise _native.SirError(f"logits have {logits.shape[1]} classes, the accumulator {self.num_classes}")
        self._ensure(logits.device)
        rc = _native.lib().sir_eval_accumulate(get_featurizer().handle, logits.data_ptr(), labels.data_ptr(), logits.shape[0],
                                               self.num_classes, self._beta.data_ptr() if self._beta is not None else None,
                                               self.n_bins, self._state.data_ptr(), self._state.numel() * 8,
                                               _native.current_stream_ptr())
        _native.check(rc, "sir_eval_accumulate")
        return self

    def state_arrays(self):
        """The state as a dict of numpy arrays -- the one device-to-host copy (it waits for the updates queued so far)."""
        return unpack_state(self._words(), self.num_classes, self.n_bins)

    def result(self, target_names=None):
        return report_from_state(self.state_arrays(), target_names)


def fit_temperature(logits, labels, iters=20):
    """Temperature scaling on a held-out split: the ``beta = 1 / T`` that minimises the mean NLL of ``softmax(beta * logits)``
    (``sir_temperature_fit``: ``iters`` safeguarded Newton steps from 1, clamped to [1/64, 64]).  Returns a float32 device
    tensor [3] = ``{beta, nll at 1, nll at beta}``; the tensor itself (its first element) is a valid ``inv_temperature``.
    Nothing is copied to the host."""
    import torch
    from . import _native
    from .featurizer import get_featurizer
    logits, labels = _logits_labels(logits, labels)
    if not (isinstance(iters, (int, np.integer)) and 0 <= iters <= 1000):
        raise _native.SirError(f"iters must be an integer in [0, 1000], got {iters!r}")
    n = logits.shape[0]
    if n > 1 << 22:
        raise _native.SirError(f"at most 2^22 rows, got {n}")
    lib = _native.lib()
    need = lib.sir_temperature_fit_workspace_bytes(n)
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=logits.device)
    out = torch.empty(3, dtype=torch.float32, device=logits.device)
    rc = lib.sir_temperature_fit(get_featurizer().handle, logits.data_ptr(), labels.data_ptr(), n, logits.shape[1], int(iters),
                                 out.data_ptr(), ws.data_ptr(), ws.numel() * 8, _native.current_stream_ptr())
    _native.check(rc, "sir_temperature_fit")
    return out
