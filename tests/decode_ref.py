"""float64 reference of sir_decode_slots (include/sir_hip.h), for tests/test_decode_host.py and tests/test_decode_gpu.py.
Written from the header's contract: per-slot log-softmax with the slot's beta, tuple scores by brute force over the table (or
over the whole product space), a stable sort by (-score, row).

``restate_f32`` states the same formulas in float32 numpy.  It is used for ONE thing: sizing the bounds of the GPU tests
(SCORE_BOUND, PROB_BOUND below) -- 4 x its worst error against float64 over the tests' own inputs, which
tests/test_decode_host.py re-measures on the CPU.

It also makes the tests' seeded inputs (``case``, ``table_rows``) and lists their shapes.
"""
import heapq
import itertools

import numpy as np

LAYOUTS = [(1,), (64,), (1, 1), (1, 63), (31, 33), (6, 14, 4), (8,) * 8]
# unconstrained decoding is checked against an enumeration of the whole product, so its layouts keep the product <= 2^16:
# (8,) * 8 has 8^8 tuples and is replaced by (4,) * 8 with exactly 2^16 (still 8 slots); (8,) * 8 itself is checked against
# ``kbest_lazy``, an exact best-first search that tests/test_decode_host.py pins to the enumeration.
PRODUCT_LAYOUTS = [(1,), (64,), (1, 1), (1, 63), (31, 33), (6, 14, 4), (4,) * 8]
BATCHES = [1, 17, 321]
TABLE_SIZES = [1, 2, 63, 64, 65, 4096]
KS = [1, 3, 8]
SCALES = [1.0, 3.0, 10.0, 30.0]           # logit scale of row b: SCALES[b % 4]
MAX_ENUM = 1 << 16

# The bounds of the GPU tests.  Measured by ``worst_restatement_errors`` over every (layout, batch, table, beta) of the parity
# sweep (tests/test_decode_host.py::test_bounds_are_four_times_the_restatement_error prints and re-checks the figures):
#   scores        worst |float32 restatement - float64| = 1.21e-4 ((8,) * 8, batch 321, 4096 rows, betas: at logit scale 30 and
#                 beta 2.25 the scores of eight slots reach the thousands, where one float32 ulp is 1.2e-4) -> 4 x = 4.9e-4
#   probabilities worst 2.72e-5 over exp(s - L) of every tuple and valid_mass: exp(s - L) carries the ABSOLUTE errors of s and of
#                 L, more than the 4e-6 * n_slots (at most 3.2e-5) of a product of per-slot probabilities -> 4 x = 1.09e-4
SCORE_BOUND = 5e-4
PROB_BOUND = 1.1e-4


def prob_bound(n_slots):
    """The project's bound on a joint confidence, 4e-6 * n_slots (tests/test_slots_gpu.py), or what normalising over a table
    needs where that is more."""
    return max(4e-6 * n_slots, PROB_BOUND)


def starts(sizes):
    return [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])]


def n_product(sizes):
    return int(np.prod([int(c) for c in sizes], dtype=object))


def beta32(betas, g):
    return 1.0 if betas is None else float(np.float32(betas[g]))


def betas_of(sizes):
    """One inverse temperature per slot, as float32 values: 0.5, 0.75, ... up to 2.25."""
    return [float(np.float32(0.5 + 0.25 * (g % 8))) for g in range(len(sizes))]


def finite_rows(logits):
    return np.isfinite(np.asarray(logits, dtype=np.float64)).all(axis=1)


# ---- float64 ------------------------------------------------------------------------------------------------------------------
def log_softmax_slots(logits, sizes, betas=None):
    """[B, total] float64: per slot log softmax((l - max l) * beta), beta the float32 value the device holds."""
    logits = np.asarray(logits, dtype=np.float64)
    out = np.empty_like(logits)
    for g, (a, c) in enumerate(zip(starts(sizes), sizes)):
        d = (logits[:, a:a + c] - logits[:, a:a + c].max(axis=1, keepdims=True)) * beta32(betas, g)
        out[:, a:a + c] = d - np.log(np.exp(d).sum(axis=1, keepdims=True))
    return out


def tuple_scores(lp, sizes, rows):
    """[B, N]: s_t = sum_g lp_g[t_g] for every table row; a row with a label outside its slot scores -inf."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, len(sizes))
    s = np.zeros((lp.shape[0], rows.shape[0]))
    bad = np.zeros(rows.shape[0], dtype=bool)
    for g, (a, c) in enumerate(zip(starts(sizes), sizes)):
        bad |= (rows[:, g] < 0) | (rows[:, g] >= c)
        s += lp[:, a + np.clip(rows[:, g], 0, c - 1)]
    s[:, bad] = -np.inf
    return s


def logsumexp(s):
    m = s.max(axis=1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return (m + np.log(np.exp(s - m).sum(axis=1, keepdims=True)))[:, 0]


def _ranked(s, rows, k, big_l):
    """Stable sort by (-score, row) -> index [B, k], labels [B, k, G], logp, prob; ranks past the valid rows are -1 / -1 / -inf / 0."""
    rows = np.asarray(rows, dtype=np.int64)
    bsz, n = s.shape
    if n <= 4096:
        order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    else:                                             # the same order, without sorting 2^16 scores per row
        order = np.empty((bsz, min(k, n)), dtype=np.int64)
        for b in range(bsz):
            neg = -s[b]
            cand = np.nonzero(neg <= np.partition(neg, k - 1)[k - 1])[0]          # ascending row: the stable sort keeps it
            order[b] = cand[np.argsort(neg[cand], kind="stable")][:k]
    top = np.take_along_axis(s, order, axis=1)
    index = np.full((bsz, k), -1, dtype=np.int64)
    labels = np.full((bsz, k, rows.shape[1]), -1, dtype=np.int64)
    logp = np.full((bsz, k), -np.inf)
    prob = np.zeros((bsz, k))
    kk = order.shape[1]
    ok = top > -np.inf
    index[:, :kk] = np.where(ok, order, -1)
    labels[:, :kk] = np.where(ok[:, :, None], rows[order], -1)
    logp[:, :kk] = top
    with np.errstate(invalid="ignore"):
        prob[:, :kk] = np.where(ok, np.exp(top - big_l[:, None]), 0.0)
    return index, labels, logp, prob


def _blank_nonfinite(logits, outs):
    bad = ~finite_rows(logits)
    for o in outs:
        o[bad] = -1 if o.dtype.kind == "i" else np.nan
    return outs


def decode_table(logits, sizes, rows, k, betas=None):
    """-> index [B, k], labels [B, k, G], logp, prob, valid_mass [B], tuple_logp [B, N] (float64 / int64)."""
    lp = log_softmax_slots(np.where(np.isfinite(logits), logits, 0.0), sizes, betas)
    s = tuple_scores(lp, sizes, rows)
    big_l = logsumexp(s)
    index, labels, logp, prob = _ranked(s, rows, k, big_l)
    return _blank_nonfinite(logits, (index, labels, logp, prob, np.exp(big_l), s))


def product_rows(sizes):
    """Every tuple of the product space, lexicographic: row t is the tuple whose mixed-radix number (slot 0 most significant) is t."""
    assert n_product(sizes) <= MAX_ENUM
    return np.asarray(list(itertools.product(*[range(c) for c in sizes])), dtype=np.int64)


def decode_product(logits, sizes, k, betas=None):
    """Unconstrained, by enumeration -> index (mixed-radix), labels, logp, prob (= exp(logp)), and every tuple's score [B, prod]."""
    rows = product_rows(sizes)
    lp = log_softmax_slots(np.where(np.isfinite(logits), logits, 0.0), sizes, betas)
    s = tuple_scores(lp, sizes, rows)
    return _blank_nonfinite(logits, _ranked(s, rows, k, np.zeros(s.shape[0])) + (s,))


def mixed_radix(labels, sizes):
    n = np.zeros(np.asarray(labels).shape[:-1], dtype=np.int64)
    for g, c in enumerate(sizes):
        n = n * c + np.asarray(labels)[..., g]
    return n


def kbest_lazy(lp_row, sizes, k):
    """The k best tuples of one row of the product space by best-first search over the slots' sorted lists (exact for any
    product size) -> list of (score, labels tuple), descending score; equal scores in no promised order."""
    lists = []
    for a, c in zip(starts(sizes), sizes):
        order = np.argsort(-lp_row[a:a + c], kind="stable")
        lists.append((order, lp_row[a:a + c][order]))
    first = tuple(0 for _ in sizes)
    score = lambda pos: float(sum(v[p] for (_, v), p in zip(lists, pos)))
    heap, seen, out = [(-score(first), first)], {first}, []
    while heap and len(out) < k:
        neg, pos = heapq.heappop(heap)
        out.append((-neg, tuple(int(o[p]) for (o, _), p in zip(lists, pos))))
        for g, c in enumerate(sizes):
            if pos[g] + 1 < c:
                nxt = pos[:g] + (pos[g] + 1,) + pos[g + 1:]
                if nxt not in seen:
                    seen.add(nxt)
                    heapq.heappush(heap, (-score(nxt), nxt))
    return out


# ---- the float32 restatement --------------------------------------------------------------------------------------------------
def restate_f32(logits, sizes, rows, betas=None):
    """The header's formulas in float32 numpy -> tuple_logp [B, N], best_prob-like exp(s - L) [B, N], valid_mass [B]: d = (l - max)
    * beta, e = exp(d), rest = the sum of e without the first maximum, lp = d - log1p(rest); s added in slot order; L = max + log of a
    sum.  (The order inside the two sums is numpy's, not the wave's: this sizes a bound, it is not a bit reference.)"""
    f = np.float32
    logits = np.asarray(logits, dtype=f)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, len(sizes))
    s = None
    for g, (a, c) in enumerate(zip(starts(sizes), sizes)):
        seg = logits[:, a:a + c]
        d = ((seg - seg.max(axis=1, keepdims=True)) * f(beta32(betas, g))).astype(f)
        e = np.exp(d).astype(f)
        e[np.arange(len(e)), np.argmax(seg, axis=1)] = f(0.0)
        lp = (d - np.log1p(e.sum(axis=1, keepdims=True, dtype=f)).astype(f)).astype(f)
        term = lp[:, rows[:, g]]
        s = term if s is None else (s + term).astype(f)
    m = s.max(axis=1, keepdims=True)
    big_l = (m + np.log(np.exp((s - m).astype(f)).astype(f).sum(axis=1, keepdims=True, dtype=f)).astype(f)).astype(f)
    return s, np.exp((s - big_l).astype(f)).astype(f), np.exp(big_l[:, 0]).astype(f)


def worst_restatement_errors(logits, sizes, rows, betas=None):
    """-> (worst |score error|, worst |probability error| over exp(s - L) of every tuple and valid_mass)."""
    s32, p32, m32 = restate_f32(logits, sizes, rows, betas)
    s = tuple_scores(log_softmax_slots(logits, sizes, betas), sizes, rows)
    big_l = logsumexp(s)
    p, mass = np.exp(s - big_l[:, None]), np.exp(big_l)
    return (float(np.abs(s32.astype(np.float64) - s).max()),
            float(max(np.abs(p32.astype(np.float64) - p).max(), np.abs(m32.astype(np.float64) - mass).max())))


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def case(sizes, batch):
    """Seeded logits float32 [batch, total]: randn scaled per row by SCALES[b % 4], so that confident rows exercise the
    log1pf tail."""
    all_layouts = LAYOUTS + [(4,) * 8]
    rng = np.random.default_rng(7000 + 100 * all_layouts.index(tuple(sizes)) + batch)
    x = rng.standard_normal((batch, int(sum(sizes))))
    return (x * np.asarray(SCALES)[np.arange(batch) % 4][:, None]).astype(np.float32)


def table_sizes(sizes):
    """The parity sweep's table sizes for a layout: the lane-stride edges that the layout has tuples for."""
    return [n for n in TABLE_SIZES if n <= n_product(sizes)]


def table_rows(sizes, n):
    """n distinct tuples drawn from the product space, in drawn (unsorted) order, int64 [n, G]."""
    total = n_product(sizes)
    rng = np.random.default_rng(9000 + 10 * n + len(sizes) + int(sum(sizes)))
    numbers = rng.choice(total, size=n, replace=False)
    rows = np.empty((n, len(sizes)), dtype=np.int64)
    for g in range(len(sizes) - 1, -1, -1):
        rows[:, g] = numbers % sizes[g]
        numbers = numbers // sizes[g]
    return rows
