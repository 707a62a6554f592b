"""float64 reference of the slot-head calls (include/sir_hip.h "slot heads"), the reference of tests/test_slots_host.py and
tests/test_slots_gpu.py.  Per slot it slices the segment and calls the UNMODIFIED single-head references --
``recipe_ref.soft_ce`` for the loss, ``eval_ref.classify`` / ``eval_ref.eval_accumulate`` for classification and evaluation;
only the joint quantities (weighted loss sum, joint confidence, the joint block of the evaluation state) are written out
here, in numpy float64.  tests/test_slots_host.py pins the loss to ``F.cross_entropy`` in torch float64.

It also makes the seeded inputs of the GPU tests (``case``) and states the conditions they must meet (``condition_margins``).
"""
import numpy as np
import torch

import eval_ref
import recipe_ref

IGNORE = -100
N_BINS = 15
LAYOUTS = [(1,), (64,), (1, 1), (1, 63), (31, 33), (6, 14, 4), (1,) * 8, (8,) * 8, (2, 2, 2, 2, 2, 2, 2, 50)]
BATCHES = [1, 17, 321, 1041]


def starts(sizes):
    return [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])]


def segments(sizes):
    return [(s, s + c) for s, c in zip(starts(sizes), sizes)]


# ---- loss ---------------------------------------------------------------------------------------------------------------------
def soft_ce_slots(logits, ya, sizes, weights=None, yb=None, lam=None, eps=0.0):
    """-> (loss, slot_losses [G], dlogits [B, sum sizes]) in float64: per slot ``recipe_ref.soft_ce`` on the segment with column g
    of the labels (smoothing eps / C_g, the mean over the rows whose slot-g label is not -100), loss = sum_g w_g slot_loss[g],
    dlogits segment g = w_g * that slot's gradient."""
    w = [1.0] * len(sizes) if weights is None else [float(v) for v in weights]
    d = torch.zeros(logits.shape, dtype=torch.float64)
    slot_losses = []
    for g, (a, b) in enumerate(segments(sizes)):
        l, dl = recipe_ref.soft_ce(logits[:, a:b], ya[:, g], None if yb is None else yb[:, g], lam, eps)
        slot_losses.append(l)
        d[:, a:b] = w[g] * dl
    slot_losses = torch.stack(slot_losses)
    return (torch.tensor(w, dtype=torch.float64) * slot_losses).sum(), slot_losses, d


# ---- classification -----------------------------------------------------------------------------------------------------------
def classify_slots(logits, sizes, k, betas=None):
    """-> probs [B, total], topk_idx int32 [B, G, k], topk_prob [B, G, k], joint [B] (float64).  Per slot ``eval_ref.classify`` with
    min(k, C_g) ranks; the ranks beyond a slot's width hold -1 / 0; a non-finite segment is NaN / -1 in all k ranks and makes
    the row's joint NaN."""
    logits = np.asarray(logits, dtype=np.float64)
    bsz, g_n = logits.shape[0], len(sizes)
    probs = np.empty_like(logits)
    idx = np.full((bsz, g_n, k), -1, dtype=np.int32)
    top = np.zeros((bsz, g_n, k))
    joint = np.ones(bsz)
    for g, (a, b) in enumerate(segments(sizes)):
        kk = min(k, b - a)
        p, i, t = eval_ref.classify(logits[:, a:b], kk, None if betas is None else betas[g])
        probs[:, a:b] = p
        idx[:, g, :kk] = i
        top[:, g, :kk] = t
        bad = ~eval_ref.finite_rows(logits[:, a:b])
        top[bad, g, :] = np.nan
        joint = joint * t[:, 0]
    return probs, idx, top, joint


# ---- evaluation ---------------------------------------------------------------------------------------------------------------
def empty_state(sizes, n_bins):
    return {"slots": [eval_ref.empty_state(c, n_bins) for c in sizes],
            "joint": {"n": 0, "exact_match": 0, "slots_correct": np.zeros(9, dtype=np.int64), "nll_sum": 0.0,
                      "bin_count": np.zeros(n_bins, dtype=np.int64), "bin_correct": np.zeros(n_bins, dtype=np.int64),
                      "bin_conf_sum": np.zeros(n_bins), "n_excluded": 0}}


def joint_terms(logits, labels, sizes, betas=None):
    """Per row, float64: counted (every slot has a valid label and a finite segment), joint confidence, the row's NLL summed
    over the slots, the number of slots whose prediction is the label (the last three only meaningful on counted rows)."""
    logits = np.asarray(logits, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    bsz = logits.shape[0]
    counted = np.ones(bsz, dtype=bool)
    for g, (a, b) in enumerate(segments(sizes)):
        counted &= eval_ref.row_kinds(logits[:, a:b], labels[:, g]) == 0
    conf, nll, right = np.ones(bsz), np.zeros(bsz), np.zeros(bsz, dtype=np.int64)
    rows = np.nonzero(counted)[0]
    for g, (a, b) in enumerate(segments(sizes)):
        if not len(rows):
            break
        l, y = logits[rows, a:b], labels[rows, g]
        p = eval_ref.softmax(l, None if betas is None else betas[g])
        pred = eval_ref.ranking(l)[:, 0]
        conf[rows] *= p[np.arange(len(rows)), pred]
        nll[rows] += -np.log(p[np.arange(len(rows)), y])
        right[rows] += (pred == y).astype(np.int64)
    return counted, conf, nll, right


def eval_accumulate_slots(state, logits, labels, sizes, n_bins, betas=None):
    """Adds one batch into ``state`` (in place): slot state g by ``eval_ref.eval_accumulate`` on segment g and column g of the
    labels; the joint block from ``joint_terms``."""
    logits = np.asarray(logits, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    for g, (a, b) in enumerate(segments(sizes)):
        eval_ref.eval_accumulate(state["slots"][g], logits[:, a:b], labels[:, g], n_bins, None if betas is None else betas[g])
    counted, conf, nll, right = joint_terms(logits, labels, sizes, betas)
    j = state["joint"]
    rows = np.nonzero(counted)[0]
    j["n"] += len(rows)
    j["n_excluded"] += int((~counted).sum())
    if len(rows):
        exact = right[rows] == len(sizes)
        bins = np.minimum(n_bins - 1, np.floor(conf[rows] * n_bins).astype(np.int64))
        j["exact_match"] += int(exact.sum())
        np.add.at(j["slots_correct"], right[rows], 1)
        j["nll_sum"] += float(nll[rows].sum())
        np.add.at(j["bin_count"], bins, 1)
        np.add.at(j["bin_correct"], bins, exact.astype(np.int64))
        np.add.at(j["bin_conf_sum"], bins, conf[rows])
    return state


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def betas_of(sizes):
    """One inverse temperature per slot, as float32 values: 0.5, 0.75, ... cycling up to 2.25."""
    return [float(np.float32(0.5 + 0.25 * (g % 8))) for g in range(len(sizes))]


def condition_margins(logits, labels, sizes, n_bins=N_BINS, betas=None):
    """What must not hang on a rounding, in float64, per row -> (gap [B], edge [B]):
    gap  = the smallest top-2 logit gap over the row's slots of width >= 2 (inf when every slot has one class);
    edge = the distance of the row's joint confidence from the nearest INTERIOR bin edge j / n_bins, 0 < j < n_bins (inf for
           n_bins == 1).  The outer edges 0 and 1 are left out on purpose: the bin index is clamped to [0, n_bins - 1], so a
           confidence of exactly 1 -- every layout of width-1 slots -- lands in the last bin whichever way the product rounds."""
    logits = np.asarray(logits, dtype=np.float64)
    gap = np.full(logits.shape[0], np.inf)
    for a, b in segments(sizes):
        if b - a >= 2:
            s = np.sort(logits[:, a:b], axis=1)
            gap = np.minimum(gap, s[:, -1] - s[:, -2])
    conf = classify_slots(logits, sizes, 1, betas)[3]
    edges = np.arange(1, n_bins) / n_bins
    edge = np.abs(conf[:, None] - edges[None, :]).min(axis=1) if n_bins > 1 else np.full(len(conf), np.inf)
    return gap, edge


GAP_MIN = 1e-4
EDGE_MIN = 1e-4 / N_BINS

# Seeds of ``case`` for which EVERY row meets the two conditions, with beta = 1 and with ``betas_of`` (found by trying
# 0, 1, 2, ... on the CPU; tests/test_slots_host.py asserts the conditions for all of them).  Missing entries use seed 0.
SEEDS = {((64,), 1041): 2, ((1, 63), 321): 1, ((1, 63), 1041): 2, ((6, 14, 4), 1041): 4}


def case(sizes, batch, second=False):
    """The seeded inputs of a (layout, batch): logits 3 * randn [B, total], labels int64 [B, G] in range, with ``second`` a
    second label set and a weight per row (0 in row 0, 1 in row 1 when they exist).  From batch 17 on, row 2 is ignored in
    slot 0 (its second label there is invalid, because it is not read) and the last row in the last slot."""
    sizes = tuple(sizes)
    g = torch.Generator().manual_seed(1000 * LAYOUTS.index(sizes) + batch + 100000 * SEEDS.get((sizes, batch), 0))
    total = sum(sizes)
    logits = torch.randn(batch, total, generator=g) * 3.0
    ya = torch.stack([torch.randint(0, c, (batch,), generator=g) for c in sizes], dim=1)
    yb = lam = None
    if second:
        yb = torch.stack([torch.randint(0, c, (batch,), generator=g) for c in sizes], dim=1)
        lam = torch.rand(batch, generator=g)
        lam[0] = 0.0
        if batch > 1:
            lam[1] = 1.0
    if batch >= 17:
        ya[2, 0] = IGNORE
        ya[batch - 1, len(sizes) - 1] = IGNORE
        if second:
            yb[2, 0] = 10 ** 6
    return logits, ya, yb, lam


def weights_of(sizes):
    """Loss weights of the tests: 1, 0.5, 2, 0.25, ... (exact in fp32)."""
    return [[1.0, 0.5, 2.0, 0.25, 1.5, 0.75, 3.0, 0.125][g] for g in range(len(sizes))]
