"""float64 numpy restatement of the prototype bank and the prototype head (include/sir_hip.h: sir_proto_accumulate,
sir_proto_finalize, sir_proto_score), taking the fp32 inputs as given, plus the bounds the tests hold the kernels to and an fp32
restatement of the score (the kernel's arithmetic in numpy) whose measured error shows the bounds have room."""
import numpy as np

DIM = 512
# With unit vectors a 512-term fp32 dot product errs, in any order, by at most 512 * 2^-24 * sum |u_i p_i| <= 3.05e-5; the fp32
# rounding of u adds a few 2^-24.
SIM_BOUND = 600.0 * 2.0 ** -24


def prob_bound(p, scale):
    """|error| allowed on a probability p = softmax(scale * s)[c] when every s errs by at most SIM_BOUND: numerator and
    denominator each move by a factor within exp(+-scale * SIM_BOUND), plus a few fp32 roundings."""
    return (np.exp(2.0 * scale * SIM_BOUND) - 1.0) * p + 4.0 * 2.0 ** -24


def unit_rows(emb):
    """emb float32 [B, 512] -> (u float64 [B, 512], ok bool [B]); ok: finite and norm > 0 (the norm in double: 1e-30 is fine)"""
    e = np.asarray(emb, dtype=np.float32).astype(np.float64)
    finite = np.isfinite(e).all(axis=1)
    e = np.where(finite[:, None], e, 0.0)
    norm = np.sqrt((e * e).sum(axis=1))
    ok = finite & (norm > 0.0)
    return np.where(ok[:, None], e / np.where(ok, norm, 1.0)[:, None], 0.0), ok


def accumulate(total, count, emb, labels):
    """sum[label] += e / ||e|| row by row in ascending order, count[label] += 1 (in place) -> the rows skipped"""
    u, ok = unit_rows(emb)
    n_classes, skipped = count.shape[0], 0
    for b, label in enumerate(np.asarray(labels, dtype=np.int64).tolist()):
        if not 0 <= label < n_classes or not ok[b]:
            skipped += 1
            continue
        total[label] += u[b]
        count[label] += 1
    return skipped


def finalize(total, count):
    """-> (protos float32 [P, 512] = fp32(sum / ||sum||), live uint8 [P]); an empty class, a zero or non-finite sum: zeros, 0"""
    total = np.asarray(total, dtype=np.float64)
    finite = np.isfinite(total).all(axis=1)
    norm = np.sqrt((np.where(finite[:, None], total, 0.0) ** 2).sum(axis=1))
    live = finite & (norm > 0.0) & (np.asarray(count) > 0)
    protos = np.where(live[:, None], total / np.where(live, norm, 1.0)[:, None], 0.0)
    return protos.astype(np.float32), live.astype(np.uint8)


def class_of(n_protos, live=None, proto_class=None, n_classes=None):
    """-> (cls int64 [P]: the class a prototype scores for, -1 if it takes no part; n_classes)"""
    cls = np.arange(n_protos, dtype=np.int64) if proto_class is None else np.asarray(proto_class, dtype=np.int64).copy()
    n_classes = n_protos if n_classes is None else n_classes
    cls[(cls < 0) | (cls >= n_classes)] = -1
    if live is not None:
        cls[np.asarray(live) == 0] = -1
    return cls, n_classes


def class_scores(sims, cls, n_classes):
    """sims [B, P] -> s [B, n_classes]: the maximum over the class's prototypes, NaN for a class with none"""
    s = np.full((n_classes, sims.shape[0]), -np.inf, dtype=sims.dtype)
    on = cls >= 0
    np.maximum.at(s, cls[on], sims[:, on].T)
    s[~np.isin(np.arange(n_classes), cls[on])] = np.nan
    return np.ascontiguousarray(s.T)


def similarities(emb, protos):
    """<e / ||e||, protos[p]> in float64 -> [B, P] (rows that cannot be scored: zeros)"""
    return unit_rows(emb)[0] @ np.asarray(protos, dtype=np.float32).astype(np.float64).T


def score(emb, protos, live=None, proto_class=None, n_classes=None, scale=1.0, k=3, sims=None):
    """The head in float64 -> dict: ``ok`` [B], ``sims`` [B, P], ``s`` [B, NC] (NaN = absent class), ``prob`` [B, NC] (0 where
    absent), ``order`` (per row the present classes by descending s, equal s by ascending class), ``cls`` [P].  ``sims``: the
    result of ``similarities`` on the same inputs, to save forming it again."""
    ok = unit_rows(emb)[1]
    sims = similarities(emb, protos) if sims is None else sims
    cls, n_classes = class_of(np.asarray(protos).shape[0], live, proto_class, n_classes)
    s = class_scores(sims, cls, n_classes)
    present = ~np.isnan(s[0]) if s.shape[0] else np.zeros((n_classes,), bool)
    prob = np.zeros_like(s)
    if present.any():
        z = scale * (s[:, present] - s[:, present].max(axis=1, keepdims=True))
        e = np.exp(z)
        prob[:, present] = e / e.sum(axis=1, keepdims=True)
    idx = np.flatnonzero(present)
    order = [idx[np.lexsort((idx, -s[b, idx]))] for b in range(s.shape[0])]
    return {"ok": ok, "sims": sims, "s": s, "prob": prob, "order": order, "cls": cls, "present": present, "k": k}


def sims_f32(emb, protos):
    """The kernel's arithmetic in numpy float32: u rounded to fp32, per lane the 8-term chain in element order (a rounded product
    and a rounded sum per term: no fma here, so this errs a little MORE than the kernel), then the butterfly over the 64 lanes."""
    u, _ = unit_rows(emb)
    u32 = u.astype(np.float32)
    p32 = np.asarray(protos, dtype=np.float32)
    out = np.empty((u32.shape[0], p32.shape[0]), np.float32)
    for b in range(u32.shape[0]):
        prod = (u32[b][None, :] * p32).reshape(p32.shape[0], 64, 8)
        acc = prod[:, :, 0]
        for i in range(1, 8):
            acc = acc + prod[:, :, i]
        width = 64
        while width > 1:
            width //= 2
            acc = acc[:, :width] + acc[:, width:2 * width]
        out[b] = acc[:, 0]
    return out


def check_ranking(ref_s, got_class, k):
    """The ranking rules for one row.  ref_s: float64 [NC], NaN = absent.  got_class: the k returned classes.  -> None or a
    message.  (1) the first min(k, present) classes are distinct present classes and the rest are -1; (2) the float64 score of
    the class at rank r is within 2 * SIM_BOUND of the reference's r-th best; (3) wherever the reference's gap between ranks r
    and r + 1 exceeds 2 * SIM_BOUND, the first r + 1 classes are the reference's."""
    present = np.flatnonzero(~np.isnan(ref_s))
    best = present[np.lexsort((present, -ref_s[present]))]
    n = min(k, len(present))
    got = [int(c) for c in got_class]
    if any(c != -1 for c in got[n:]):
        return f"ranks beyond the {len(present)} present classes are not -1: {got}"
    head = got[:n]
    if len(set(head)) != n or any(c not in set(present.tolist()) for c in head):
        return f"returned classes are not distinct present classes: {got}"
    for r in range(n):
        if abs(ref_s[head[r]] - ref_s[best[r]]) > 2 * SIM_BOUND:
            return f"rank {r}: class {head[r]} scores {ref_s[head[r]]}, the reference's rank {r} scores {ref_s[best[r]]}"
        gap = ref_s[best[r]] - ref_s[best[r + 1]] if r + 1 < len(best) else np.inf
        if gap > 2 * SIM_BOUND and set(head[:r + 1]) != set(best[:r + 1].tolist()):
            return f"the first {r + 1} classes {head[:r + 1]} are not the reference's {best[:r + 1].tolist()}"
    return None
