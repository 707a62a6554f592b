"""float64 numpy restatement of sir_classify, sir_eval_accumulate and sir_temperature_fit (include/sir_hip.h), the
reference of tests/test_eval_host.py and tests/test_eval_gpu.py.  Written from the header's contract, not from the kernels:
plain loops and sorts, no wave tricks.  ``temperature_fit(..., dtype=np.float32)`` runs the same Newton iteration with
the per-row terms in float32 (sums over rows still in double), which is how the GPU tolerance is measured."""
import numpy as np

IGNORE = -100
TOPK_SLOTS = 8


def finite_rows(logits):
    return np.isfinite(np.asarray(logits, dtype=np.float64)).all(axis=1)


def ranking(logits):
    """[B, C] class indices by descending logit, equal logits by ascending index (a stable sort of the negated row)."""
    logits = np.asarray(logits, dtype=np.float64)
    return np.argsort(-logits, axis=1, kind="stable")


def softmax(logits, beta=None):
    """float64 softmax of logits * beta with the row maximum subtracted; beta is the float32 value the device holds."""
    v = np.asarray(logits, dtype=np.float64) * (1.0 if beta is None else float(np.float32(beta)))
    v = v - v.max(axis=1, keepdims=True)
    e = np.exp(v)
    return e / e.sum(axis=1, keepdims=True)


def classify(logits, k, beta=None):
    """-> probs [B, C], topk_idx int32 [B, k], topk_prob [B, k]; a row with a NaN or an infinity is NaN / -1."""
    logits = np.asarray(logits, dtype=np.float64)
    b, c = logits.shape
    assert 1 <= k <= min(8, c)
    ok = finite_rows(logits)
    probs = np.full((b, c), np.nan)
    idx = np.full((b, k), -1, dtype=np.int32)
    top = np.full((b, k), np.nan)
    if ok.any():
        p = softmax(logits[ok], beta)
        order = ranking(logits[ok])[:, :k]
        probs[ok] = p
        idx[ok] = order
        top[ok] = np.take_along_axis(p, order, axis=1)
    return probs, idx, top


def empty_state(num_classes, n_bins):
    return {"confusion": np.zeros((num_classes, num_classes), dtype=np.int64), "n": 0,
            "topk_correct": np.zeros(TOPK_SLOTS, dtype=np.int64), "nll_sum": 0.0,
            "bin_count": np.zeros(n_bins, dtype=np.int64), "bin_correct": np.zeros(n_bins, dtype=np.int64),
            "bin_conf_sum": np.zeros(n_bins, dtype=np.float64), "n_ignored": 0, "n_nonfinite": 0}


def row_kinds(logits, labels):
    """0 counted, 1 ignored (-100), 2 label outside [0, C), 3 non-finite row -- looked at in that order."""
    labels = np.asarray(labels, dtype=np.int64)
    c = np.asarray(logits).shape[1]
    kinds = np.where(finite_rows(logits), 0, 3)
    kinds = np.where((labels < 0) | (labels >= c), 2, kinds)
    return np.where(labels == IGNORE, 1, kinds)


def confidences(logits, beta=None):
    """p_max of every row in float64 (rows must be finite)."""
    return softmax(logits, beta).max(axis=1)


def eval_accumulate(state, logits, labels, n_bins, beta=None):
    """Adds one batch into ``state`` (in place) and returns it, with ``bad_label`` = the batch held a label that raises."""
    logits = np.asarray(logits, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    c = logits.shape[1]
    kinds = row_kinds(logits, labels)
    state["n_ignored"] += int((kinds == 1).sum())
    state["n_nonfinite"] += int((kinds == 3).sum())
    state["bad_label"] = bool(state.get("bad_label", False) or (kinds == 2).any())
    rows = np.nonzero(kinds == 0)[0]
    if len(rows):
        l, y = logits[rows], labels[rows]
        p = softmax(l, beta)
        order = ranking(l)
        pred = order[:, 0]
        rank_y = np.argmax(order == y[:, None], axis=1)
        pmax = p[np.arange(len(rows)), pred]
        bins = np.minimum(n_bins - 1, np.floor(pmax * n_bins).astype(np.int64))
        np.add.at(state["confusion"], (y, pred), 1)
        state["n"] += len(rows)
        for j in range(TOPK_SLOTS):
            state["topk_correct"][j] += int((rank_y < min(j + 1, c)).sum())
        state["nll_sum"] += float(-np.log(p[np.arange(len(rows)), y]).sum())
        np.add.at(state["bin_count"], bins, 1)
        np.add.at(state["bin_correct"], bins, (pred == y).astype(np.int64))
        np.add.at(state["bin_conf_sum"], bins, pmax)
    return state


def nll(logits, labels, beta):
    """f(beta) = mean_i [logsumexp(beta l_i) - beta l_{i, y_i}] over the counted rows, float64."""
    logits = np.asarray(logits, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    rows = np.nonzero(row_kinds(logits, labels) == 0)[0]
    v = logits[rows] * float(beta)
    m = v.max(axis=1)
    lse = m + np.log(np.exp(v - m[:, None]).sum(axis=1))
    return float(np.mean(lse - v[np.arange(len(rows)), labels[rows]]))


def _fit_terms(l, y, beta, dtype):
    """Per-row f, f', f'' terms at beta in ``dtype`` on the centred logits c = l - max l (the maximum subtracted first),
    summed over rows in double."""
    beta = dtype(beta)
    c = l - l.max(axis=1, keepdims=True)
    e = np.exp(c * beta)
    den = e.sum(axis=1, keepdims=True, dtype=dtype)
    mean = (e * c).sum(axis=1, keepdims=True, dtype=dtype) / den
    var = (e * (c - mean) ** 2).sum(axis=1, keepdims=True, dtype=dtype) / den
    idx = np.arange(len(y))
    f = np.log(den[:, 0]) - c[idx, y] * beta
    g = mean[:, 0] - c[idx, y]
    return (float(f.astype(np.float64).sum()), float(g.astype(np.float64).sum()), float(var[:, 0].astype(np.float64).sum()))


def temperature_fit(logits, labels, iters=20, dtype=np.float64):
    """The safeguarded Newton iteration of sir_temperature_fit -> (beta, nll at 1, nll at beta), the two nll as the
    iteration itself evaluates them.  ``dtype=np.float64``: everything in double, beta never rounded.
    ``dtype=np.float32``: per-row terms in float32 and beta rounded to float32 after every step, as on the device."""
    logits = np.asarray(logits)
    labels = np.asarray(labels, dtype=np.int64)
    rows = np.nonzero(row_kinds(logits, labels) == 0)[0]
    n = len(rows)
    if n == 0:
        return 1.0, float("nan"), float("nan")
    l = logits[rows].astype(dtype)
    y = labels[rows]
    beta = 1.0
    f1 = None
    for _ in range(iters):
        fs, gs, hs = _fit_terms(l, y, beta, dtype)
        if f1 is None:
            f1 = fs / n
        g, h = gs / n, hs / n
        b = beta - g / max(h, 1e-12)
        b = min(max(b, 0.5 * beta), 2.0 * beta)
        b = min(max(b, 1.0 / 64.0), 64.0)
        beta = float(dtype(b))
    fb = _fit_terms(l, y, beta, dtype)[0] / n
    return beta, (fb if f1 is None else f1), fb


def confusion_and_report(y_true, y_pred, num_classes):
    """Confusion matrix and sklearn-layout report of hard predictions, through the same host code the library uses on a
    state (sir_amd.metrics.classification_from_confusion), so that the host test pins that code to sklearn."""
    from sir_amd import metrics
    cm = np.zeros((num_classes, num_classes), dtype=np.int64)
    np.add.at(cm, (np.asarray(y_true, dtype=np.int64), np.asarray(y_pred, dtype=np.int64)), 1)
    return cm, metrics.classification_from_confusion(cm)
