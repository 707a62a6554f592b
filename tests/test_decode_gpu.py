"""GPU: joint decoding of the slot heads -- sir_decode_slots (include/sir_hip.h) and what stands on it.

1. parity with the float64 reference (tests/decode_ref.py) over the wave / workgroup / lane-stride edges, constrained and
   unconstrained, with and without per-slot betas, logit scales 1 .. 30;
2. exact properties (against sir_classify_slots, constrained over the full table against unconstrained, ties, reproducibility);
3. the row kinds (non-finite segment, width-1 slot, a table byte out of range);
4. refused calls write nothing;
5. the Python surface (result dictionaries, streams, scripts/evaluate.py).

Bounds: ``decode_ref.SCORE_BOUND`` on scores and ``decode_ref.prob_bound`` on probabilities, both sized from the float32
restatement of the formulas at 4 x margin (tests/test_decode_host.py measures them on the CPU).  Rankings are checked without
leaving a case out: the returned tuples are distinct rows of the table, the float64 score of the tuple at rank r is within
2 x SCORE_BOUND of the reference's r-th best score, and wherever the reference's gap between ranks r and r + 1 exceeds
2 x SCORE_BOUND the first r + 1 tuples are the reference's first r + 1 (so a rank with such a gap on both sides is the
reference's tuple itself).  The (8,) * 8 layout has 8^8 tuples, beyond what the reference enumerates: unconstrained decoding is
swept over (4,) * 8 (2^16 tuples) in its place and checked on (8,) * 8 against ``decode_ref.kbest_lazy``."""
import ctypes as C
import json
import types

import numpy as np
import pandas as pd
import pytest
import torch

import decode_ref as R
from sir_amd import _native, ops, slots
from sir_amd.featurizer import get_featurizer

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0
FSC = (6, 14, 4)


def _id(sizes):
    return "x".join(map(str, sizes)) if len(set(sizes)) > 1 else f"{sizes[0]}x{len(sizes)}"


def _table_dev(rows, n_slots):
    return torch.from_numpy(slots.pack_tuples(rows, n_slots)).to(DEV)


def _beta_dev(betas):
    return None if betas is None else torch.tensor(betas, dtype=torch.float32, device=DEV)


def _raw(lg, sizes, k, beta=None, table=None, n=None, mass=True, scores=None, n_slots=None, num_classes=None, table_ptr=None):
    """One sir_decode_slots call with every output pre-filled with a sentinel -> (rc, index, labels, logp, prob, mass, scores)."""
    b, g = lg.shape[0], len(sizes)
    n = (0 if table is None else table.shape[0]) if n is None else n
    scores = (table is not None) if scores is None else scores
    kk = max(min(k, 8), 1)
    index = torch.full((b, kk), -7, dtype=torch.int32, device=DEV)
    labels = torch.full((b, kk, g), -7, dtype=torch.int32, device=DEV)
    logp, prob = torch.full((b, kk), SENT, device=DEV), torch.full((b, kk), SENT, device=DEV)
    mass_t = torch.full((b,), SENT, device=DEV)
    scores_t = torch.full((b, max(n, 1)), SENT, device=DEV)
    if table_ptr is None:
        table_ptr = table.data_ptr() if table is not None else None
    rc = _native.lib().sir_decode_slots(get_featurizer().handle, lg.data_ptr(), b, lg.shape[1] if num_classes is None else num_classes,
                                        (C.c_int32 * g)(*sizes), g if n_slots is None else n_slots,
                                        beta.data_ptr() if beta is not None else None, table_ptr, n, k, index.data_ptr(), labels.data_ptr(),
                                        logp.data_ptr(), prob.data_ptr(), mass_t.data_ptr() if mass else None,
                                        scores_t.data_ptr() if scores else None, _native.current_stream_ptr())
    return rc, index, labels, logp, prob, mass_t, scores_t


def _np(*ts):
    return [t.cpu().numpy() for t in ts]


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------
def _check_ranks(got, rows, s64, big_l, ref_logp, k, n_slots, what):
    """``got``: (index, labels, logp, prob) of the device as numpy; rows [N, G] the table; s64 [B, N] its float64 scores; big_l [B]
    the float64 normaliser (0: unconstrained); ref_logp [B, >= k + 1] the reference's sorted scores (-inf past the table)."""
    index, labels, logp, prob = got
    n = rows.shape[0]
    live = min(k, n)
    pb = R.prob_bound(n_slots)
    assert (index[:, live:] == -1).all() and (labels[:, live:] == -1).all(), what
    assert np.isneginf(logp[:, live:]).all() and (prob[:, live:] == 0).all(), what
    idx = index[:, :live].astype(np.int64)
    assert ((idx >= 0) & (idx < n)).all(), what
    srt = np.sort(idx, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), f"{what}: a tuple twice"
    assert np.array_equal(labels[:, :live], rows[idx]), what
    mine = np.take_along_axis(s64, idx, axis=1)                                           # float64 scores of the returned tuples
    rank_err = np.abs(mine - ref_logp[:, :live]).max()
    score_err = np.abs(logp[:, :live].astype(np.float64) - mine).max()
    prob_err = np.abs(prob[:, :live].astype(np.float64) - np.exp(mine - big_l[:, None])).max()
    print(f"{what} k={k}: rank score diff {rank_err:.2e} (bound {2 * R.SCORE_BOUND:.1e}), best_logp err {score_err:.2e} "
          f"(bound {R.SCORE_BOUND:.1e}), best_prob err {prob_err:.2e} (bound {pb:.1e})")
    assert rank_err <= 2 * R.SCORE_BOUND and score_err <= R.SCORE_BOUND and prob_err <= pb, what
    return idx


def _check_sets(idx, ref_index, ref_logp, n, what):
    """Where the reference's gap behind rank r exceeds 2 x SCORE_BOUND (or the table ends there), the first r + 1 tuples are the
    reference's first r + 1."""
    live = idx.shape[1]
    for r in range(live):
        clear = np.ones(idx.shape[0], dtype=bool) if r + 1 >= n else (ref_logp[:, r] - ref_logp[:, r + 1] > 2 * R.SCORE_BOUND)
        a, b = np.sort(idx[clear, :r + 1], axis=1), np.sort(ref_index[clear, :r + 1], axis=1)
        assert np.array_equal(a, b), f"{what}: ranks 0..{r}"


@pytest.mark.parametrize("sizes", R.LAYOUTS, ids=_id)
@pytest.mark.parametrize("batch", R.BATCHES)
def test_constrained_decoding_matches_float64(sizes, batch):
    x = R.case(sizes, batch)
    lg = torch.from_numpy(x).to(DEV)
    for n in R.table_sizes(sizes):
        rows = R.table_rows(sizes, n)
        table = _table_dev(rows, len(sizes))
        for betas in (None, R.betas_of(sizes)):
            ref_index, _, ref_logp, _, ref_mass, s64 = R.decode_table(x, sizes, rows, 9, betas)
            big_l = R.logsumexp(s64)
            for k in R.KS:                                                                # (k > n at n = 1, 2: the padding)
                rc, *outs = _raw(lg, sizes, k, _beta_dev(betas), table)
                assert rc == 0
                index, labels, logp, prob, mass, scores = _np(*outs)
                what = f"table {_id(sizes)} B={batch} n={n} betas={'set' if betas else None}"
                idx = _check_ranks((index, labels, logp, prob), rows, s64, big_l, ref_logp, k, len(sizes), what)
                _check_sets(idx, ref_index, ref_logp, n, what)
                mass_err = np.abs(mass.astype(np.float64) - ref_mass).max()
                all_err = np.abs(scores.astype(np.float64) - s64).max()
                print(f"{what} k={k}: valid_mass err {mass_err:.2e}, tuple_logp err {all_err:.2e}")
                assert mass_err <= R.prob_bound(len(sizes)) and all_err <= R.SCORE_BOUND, what
    ops.check_status()


@pytest.mark.parametrize("sizes", R.PRODUCT_LAYOUTS, ids=_id)
@pytest.mark.parametrize("batch", R.BATCHES)
def test_unconstrained_decoding_matches_the_enumerated_product(sizes, batch):
    x = R.case(sizes, batch)
    lg = torch.from_numpy(x).to(DEV)
    rows = R.product_rows(sizes)
    for betas in (None, R.betas_of(sizes)):
        ref_index, _, ref_logp, _, s64 = R.decode_product(x, sizes, 9, betas)
        for k in R.KS:
            rc, *outs = _raw(lg, sizes, k, _beta_dev(betas))
            assert rc == 0
            index, labels, logp, prob, mass, _ = _np(*outs)
            what = f"product {_id(sizes)} B={batch} betas={'set' if betas else None}"
            idx = _check_ranks((index, labels, logp, prob), rows, s64, np.zeros(batch), ref_logp, k, len(sizes), what)
            _check_sets(idx, ref_index, ref_logp, rows.shape[0], what)
            assert (mass == 1.0).all()
    ops.check_status()


def test_unconstrained_decoding_of_eight_slots_of_eight():
    """8^8 tuples: the reference is the exact best-first search; best_index is the mixed-radix number, up to 8^8 - 1."""
    sizes, batch = (8,) * 8, 17
    x = R.case(sizes, batch)
    betas = R.betas_of(sizes)
    lp = R.log_softmax_slots(x, sizes, betas)
    rc, *outs = _raw(torch.from_numpy(x).to(DEV), sizes, 8, _beta_dev(betas))
    assert rc == 0
    index, labels, logp, prob, _, _ = _np(*outs)
    st = R.starts(sizes)
    for b in range(batch):
        want = R.kbest_lazy(lp[b], sizes, 9)
        assert len({tuple(r) for r in labels[b].tolist()}) == 8
        for r in range(8):
            mine = sum(lp[b, st[g] + labels[b, r, g]] for g in range(8))
            assert abs(mine - want[r][0]) <= 2 * R.SCORE_BOUND and abs(float(logp[b, r]) - mine) <= R.SCORE_BOUND
            assert abs(float(prob[b, r]) - np.exp(mine)) <= R.prob_bound(8)
            if want[r][0] - want[r + 1][0] > 2 * R.SCORE_BOUND:
                assert {tuple(v) for v in labels[b, :r + 1].tolist()} == {w[1] for w in want[:r + 1]}
    assert np.array_equal(index, R.mixed_radix(labels, sizes)) and index.max() < 8 ** 8


# ---- 2. exact properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", R.LAYOUTS, ids=_id)
def test_unconstrained_rank_0_is_the_independent_argmax(sizes):
    x = R.case(sizes, 321)
    lg = torch.from_numpy(x).to(DEV)
    for betas in (None, R.betas_of(sizes)):
        idx, _, joint = slots.classify(lg, sizes, k=1, inv_temperature=betas)
        rc, index, labels, logp, prob, _, _ = _raw(lg, sizes, 1, _beta_dev(betas))
        assert rc == 0 and torch.equal(labels[:, 0, :], idx[:, :, 0])
        err = (prob[:, 0].double() - joint.double()).abs().max().item()
        print(f"{_id(sizes)}: |best_prob - joint_prob| {err:.2e} (bound {4e-6 * len(sizes):.1e})")
        assert err <= 4e-6 * len(sizes)


@pytest.mark.parametrize("sizes", [(1,), (64,), (1, 1), (1, 63), (31, 33), (6, 14, 4), (4,) * 6], ids=_id)
def test_constrained_over_the_full_table_has_the_unconstrained_bits(sizes):
    all_layouts = R.LAYOUTS + [(4,) * 8]
    x = R.case(sizes, 321) if sizes in all_layouts else (np.random.default_rng(3).standard_normal((321, sum(sizes))) * 5).astype(np.float32)
    lg = torch.from_numpy(x).to(DEV)
    full = slots.TupleTable.full(sizes)
    for betas in (None, R.betas_of(sizes)):
        a = slots.decode(lg, sizes, table=full, k=8, inv_temperature=betas, want_mass=True)
        b = slots.decode(lg, sizes, k=8, inv_temperature=betas)
        assert torch.equal(a[2], b[2])                                                    # best_logp, bit for bit
        err = (a[4].double() - 1.0).abs().max().item()
        print(f"{_id(sizes)}: |valid_mass - 1| over the full table {err:.2e} (bound {R.prob_bound(len(sizes)):.1e})")
        assert err <= R.prob_bound(len(sizes))
        live = min(8, len(full))
        assert (a[0][:, live:] == -1).all() and (b[0][:, live:] == -1).all()


def test_an_all_zero_row_returns_the_first_rows_and_the_first_tuples():
    lg = torch.zeros((5, 24), device=DEV)
    rows = R.table_rows(FSC, 65)
    rc, index, labels, logp, prob, mass, _ = _raw(lg, FSC, 8, None, _table_dev(rows, 3))
    assert rc == 0 and (index.cpu() == torch.arange(8, dtype=torch.int32)).all()
    assert np.array_equal(labels.cpu().numpy()[0], rows[:8]) and (prob == prob[0, 0]).all() and abs(prob[0, 0].item() - 1 / 65) < 1e-6
    assert abs(mass[0].item() - 65 / 336) < 1e-6
    rc, index, labels, logp, prob, _, _ = _raw(lg, FSC, 8)
    assert rc == 0 and (index.cpu() == torch.arange(8, dtype=torch.int32)).all()
    assert np.array_equal(labels.cpu().numpy()[2], R.product_rows(FSC)[:8]) and (logp == logp[0, 0]).all()


def test_equal_scores_go_to_the_lower_row():
    sizes = (8, 8)
    seg = torch.tensor([0.5, -1.25, 3.0, 0.75, -2.0, 2.5, 0.0, 1.0])
    lg = torch.cat([seg, seg]).repeat(3, 1).to(DEV)                                       # two byte-identical segments
    for rows in ([(3, 5), (5, 3), (2, 2)], [(5, 3), (3, 5), (2, 2)]):
        rc, index, labels, logp, prob, _, _ = _raw(lg, sizes, 3, None, _table_dev(np.asarray(rows), 2))
        assert rc == 0 and index[0].tolist() == [2, 0, 1] and torch.equal(logp[:, 1], logp[:, 2]) and torch.equal(prob[:, 1], prob[:, 2])
        assert labels[0, 1].tolist() == list(rows[0])
    # unconstrained: the candidate order -- (2, 5) and (5, 2) tie behind (2, 2); slot 0's label 2 is the better partial
    rc, index, labels, logp, _, _, _ = _raw(lg, sizes, 3)
    assert rc == 0 and labels[1].tolist() == [[2, 2], [2, 5], [5, 2]] and torch.equal(logp[:, 1], logp[:, 2])


def test_two_runs_give_equal_bytes():
    x = torch.from_numpy(R.case(FSC, 321)).to(DEV)
    table = _table_dev(R.table_rows(FSC, 65), 3)
    beta = _beta_dev(R.betas_of(FSC))
    for tab in (table, None):
        a, b = _raw(x, FSC, 3, beta, tab), _raw(x, FSC, 3, beta, tab)
        used = range(1, 7) if tab is not None else range(1, 6)
        assert all(torch.equal(a[i].view(torch.int32), b[i].view(torch.int32)) for i in used)


# ---- 3. row kinds -------------------------------------------------------------------------------------------------------------
def test_a_non_finite_segment_blanks_its_row_only():
    x = R.case(FSC, 17)
    table = _table_dev(R.table_rows(FSC, 65), 3)
    bad = x.copy()
    bad[3, 7] = np.nan                                                                    # slot 1
    bad[9, 23] = np.inf                                                                   # slot 2, last column
    bad[12, 0] = -np.inf                                                                  # slot 0, first column
    hit, good = [3, 9, 12], [b for b in range(17) if b not in (3, 9, 12)]
    for tab in (table, None):
        clean = _raw(torch.from_numpy(x).to(DEV), FSC, 3, None, tab)
        rc, index, labels, logp, prob, mass, scores = _raw(torch.from_numpy(bad).to(DEV), FSC, 3, None, tab)
        assert rc == 0 and (index[hit] == -1).all() and (labels[hit] == -1).all()
        assert torch.isnan(logp[hit]).all() and torch.isnan(prob[hit]).all() and torch.isnan(mass[hit]).all()
        for got, want in zip((index, labels, logp, prob, mass), clean[1:6]):
            assert torch.equal(got[good], want[good])
        if tab is not None:
            assert torch.isnan(scores[hit]).all() and torch.equal(scores[good], clean[6][good])
    ops.check_status()


def test_a_width_one_slot_adds_nothing():
    x = R.case((1, 63), 17)
    lg = torch.from_numpy(x).to(DEV)
    a = slots.decode(lg, (1, 63), k=8)
    b = slots.decode(lg[:, 1:].contiguous(), (63,), k=8)
    assert (a[1][:, :, 0] == 0).all() and torch.equal(a[1][:, :, 1], b[1][:, :, 0]) and torch.equal(a[2], b[2]) and torch.equal(a[0], b[0])
    one = slots.decode(lg[:, :1].contiguous(), (1,), table=slots.TupleTable.full((1,)), k=3, want_mass=True)
    assert (one[0][:, 0] == 0).all() and (one[0][:, 1:] == -1).all() and (one[3][:, 0] == 1).all() and (one[4] == 1).all()


def test_a_table_byte_out_of_range_is_flagged_and_never_chosen():
    x = R.case(FSC, 17)
    lg = torch.from_numpy(x).to(DEV)
    rows = R.table_rows(FSC, 65)
    clean = _raw(lg, FSC, 8, None, _table_dev(rows, 3))
    ops.check_status()
    p = 10
    for bad_tuple in ((2, 14, 1), (6, 0, 0), (0, 0, 255)):
        packed = slots.pack_tuples(rows, 3)
        packed = np.concatenate([packed[:p], np.asarray([list(bad_tuple) + [0] * 5], dtype=np.uint8), packed[p:]])
        rc, index, labels, logp, prob, mass, scores = _raw(lg, FSC, 8, None, torch.from_numpy(packed).to(DEV))
        assert rc == 0
        with pytest.raises(_native.SirError):
            ops.check_status()
        ops.check_status()                                                                # (reported once, then cleared)
        moved = clean[1] + (clean[1] >= p).to(torch.int32)                                # the rows behind the bad one moved up by one
        assert torch.equal(index, moved) and torch.equal(labels, clean[2]) and torch.equal(logp, clean[3])
        assert torch.isneginf(scores[:, p]).all() and torch.equal(scores[:, :p], clean[6][:, :p]) and torch.equal(scores[:, p + 1:], clean[6][:, p:])
        pb = R.prob_bound(3)                                                              # (the sum's lane order changed: not bits)
        assert (prob - clean[4]).abs().max().item() <= pb and (mass - clean[5]).abs().max().item() <= pb
    # nothing valid left: every rank is padded and no mass exists
    rc, index, labels, logp, prob, mass, scores = _raw(lg, FSC, 3, None, torch.tensor([[0, 14, 0, 0, 0, 0, 0, 0]], dtype=torch.uint8, device=DEV))
    assert rc == 0 and (index == -1).all() and (labels == -1).all() and torch.isneginf(logp).all() and (prob == 0).all() and (mass == 0).all()
    with pytest.raises(_native.SirError):
        ops.check_status()
    # a byte behind the last slot is padding: it is not read
    packed = slots.pack_tuples(rows, 3)
    packed[:, 3:] = 255
    again = _raw(lg, FSC, 8, None, torch.from_numpy(packed).to(DEV))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again[1:], clean[1:]))
    ops.check_status()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    lg = torch.from_numpy(R.case(FSC, 17)).to(DEV)
    big = torch.zeros((4100, 8), dtype=torch.uint8, device=DEV)                            # (room for every n tried below)
    EINVAL = _native.SIR_EINVAL

    def untouched(outs):
        return all(bool((t == (SENT if t.is_floating_point() else -7)).all()) for t in outs)

    refused = [dict(k=0, table=big, n=65), dict(k=9, table=big, n=65), dict(k=0), dict(k=9),
               dict(k=3, table=big, n=0), dict(k=3, table=big, n=4097), dict(k=3, table=big, n=-1),
               dict(k=3, table=big, n=65, table_ptr=big.data_ptr() + 4), dict(k=3, table=big, n=65, table_ptr=big.data_ptr() + 1),
               dict(k=3, scores=True), dict(k=3, n=5),
               dict(k=3, table=big, n=65, sizes=(6, 14, 5)), dict(k=3, sizes=(6, 14, 3)), dict(k=3, n_slots=0), dict(k=3, num_classes=65),
               dict(k=3, sizes=(3,) * 9, num_classes=27)]
    for kw in refused:
        kw = dict(kw)
        rc, *outs = _raw(lg, kw.pop("sizes", FSC), kw.pop("k"), None, **kw)
        assert rc == EINVAL and untouched(outs), kw
    rc, *outs = _raw(lg, FSC, 3, None, big, n=4096)                                        # the largest table is served
    assert rc == 0 and not untouched(outs[:4])
    torch.cuda.synchronize()
    ops.check_status()


# ---- 5. through the surface ---------------------------------------------------------------------------------------------------
def _fsc_spec():
    return slots.SlotSpec(["action", "object", "location"],
                          [["activate", "bring", "change", "deactivate", "decrease", "increase"], [f"o{i}" for i in range(14)],
                           ["bedroom", "kitchen", "none", "washroom"]])


def test_joint_result_dictionaries_agree_with_the_reference():
    from sir_amd.scripts import classify_results
    spec = _fsc_spec()
    x = R.case(FSC, 17)
    x[4, 3] = np.nan
    rows = R.table_rows(FSC, 31)
    table = slots.TupleTable(spec, rows.tolist())
    betas = [1.0, 0.5, 2.0]
    lg = torch.from_numpy(x).to(DEV)
    res = classify_results.results_from_slot_logits(lg, spec, k=3, inv_temperature=betas, min_confidence=0.6, table=table, decode="joint")
    ref_index, ref_labels, ref_logp, ref_prob, ref_mass, _ = R.decode_table(x, FSC, rows, 4, betas)
    assert len(res) == 17
    pb = R.prob_bound(3)
    for b, r in enumerate(res):
        if b == 4:
            assert r["action"] == "Unknown" and np.isnan(r["confidence"]) and r["rejected"] is True and np.isnan(r["valid_mass"])
            continue
        assert "slot_confidence" not in r and len(r["top_predictions"]) == 3
        assert abs(r["confidence"] - ref_prob[b, 0]) <= pb and abs(r["valid_mass"] - ref_mass[b]) <= pb
        assert r["rejected"] == (not (r["confidence"] >= 0.6))
        assert r["top_predictions"][0]["probability"] == r["confidence"]
        for j, e in enumerate(r["top_predictions"]):
            assert abs(e["probability"] - ref_prob[b, j]) <= pb
            if (j == 0 or ref_logp[b, j - 1] - ref_logp[b, j] > 2 * R.SCORE_BOUND) and ref_logp[b, j] - ref_logp[b, j + 1] > 2 * R.SCORE_BOUND:
                assert e["slots"] == spec.decode(ref_labels[b, j]) and e["label"] == f"{e['slots']['action']}_{e['slots']['object']}"
        assert {c: r[c] for c in spec.columns} == r["top_predictions"][0]["slots"] and r["predicted_label"] == r["top_predictions"][0]["label"]
        assert tuple(spec._index[g][r[c]] for g, c in enumerate(spec.columns)) in table.index     # an intent that exists
    flags = [r["rejected"] for r in res]
    assert any(flags) and not all(flags)                                                  # the threshold cuts through this batch
    # unconstrained joint decoding: the independent argmax and the joint confidence, no valid_mass; the default is unchanged
    free = classify_results.results_of(lg, {}, spec, [1.0, 2.0, 0.5], None, None, "joint")
    plain = classify_results.results_of(lg, {}, spec, [1.0, 2.0, 0.5], None)
    for b in range(17):
        if b != 4:
            assert "valid_mass" not in free[b] and {c: free[b][c] for c in spec.columns} == {c: plain[b][c] for c in spec.columns}
            assert abs(free[b]["confidence"] - plain[b]["confidence"]) <= 4e-6 * 3
    assert "slot_confidence" in plain[0] and isinstance(plain[0]["top_predictions"], dict)
    with pytest.raises(ValueError):
        classify_results.results_of(lg, {}, spec, None, None, table)                      # a table without decode="joint"
    with pytest.raises(ValueError):
        classify_results.results_of(lg[:, :6].contiguous(), {i: str(i) for i in range(6)}, None, None, None, None, "joint")
    ops.check_status()


def test_stream_session_with_slots_equals_recognize_recordings():
    """the recordings of test_stream_gpu.py::test_stream_session_end_to_end_equals_recognize_recordings, a 24-logit model read as
    (6, 14, 4): independent, joint and table-constrained dictionaries are those of the batch route"""
    from sir_amd import synth
    from sir_amd.models.models import CNNAudioGRU
    from sir_amd.scripts.testing import IntentRecognizer
    utt = synth.synth_clips(4, 40000, seed=77).numpy()
    z = lambda chunks: np.zeros(chunks * 1024, dtype=np.float32)
    recs = [np.concatenate([z(8), utt[0, :24 * 1024], z(24), utt[1, :32 * 1024], z(20)]),
            np.concatenate([utt[2, :16 * 1024], z(32), utt[3, :5 * 1024], z(8)])]
    torch.manual_seed(5)
    model = CNNAudioGRU(24).to(DEV).eval()
    reco = IntentRecognizer.from_model(model, {f"intent_{i}": i for i in range(24)}, DEV)
    spec = _fsc_spec()
    table = slots.TupleTable(spec, R.table_rows(FSC, 31).tolist())
    for kw in (dict(slots=spec), dict(slots=spec, decode="joint", min_confidence=0.2), dict(slots=spec, tuples=table, decode="joint", temperature=[1.0, 2.0, 0.5])):
        want = reco.recognize_recordings(recs, pad_to=200, **kw)
        assert [len(f) for f in want] == [2, 2]
        session = reco.open_streams(2, max_push=1000, pad_to=200, **kw)
        found = [[], []]
        for k in range(-(-max(len(r) for r in recs) // 1000)):
            chunks = {s: r[k * 1000:(k + 1) * 1000] for s, r in enumerate(recs) if k * 1000 < len(r)}
            close = [s for s, r in enumerate(recs) if k * 1000 < len(r) <= (k + 1) * 1000]
            for u in session.feed(chunks, close=close):
                found[u["stream"]].append(u)
        assert [len(f) for f in found] == [2, 2]
        for u, w in zip([u for f in found for u in f], [w for f in want for w in f]):
            assert set(spec.columns) <= set(u) and {k: v for k, v in u.items() if k not in ("stream", "forced")} == w
            assert ("valid_mass" in u) == ("tuples" in kw) and ("rejected" in u) == ("min_confidence" in kw)
    with pytest.raises(ValueError):
        reco.open_streams(2, tuples=table, decode="joint")                                # a table without a slot layout
    ops.check_status()


def test_evaluate_writes_constrained_metrics(tmp_path):
    from sir_amd import synth
    from sir_amd.scripts import evaluate as ev
    from sir_amd.scripts import precompute_features as pf
    from test_pipeline_gpu import _make_corpus

    rows = _make_corpus(str(tmp_path / "wav"))
    for i, r in enumerate(rows):
        r["action"], r["object"] = r["label"].split("_")
        r["location"] = ["kitchen", "bedroom", "none"][i % 3]
    csv = tmp_path / "valid_data.csv"
    frame = pd.DataFrame(rows[:16])
    frame.to_csv(csv, index=False)
    pf.precompute_dataset_features(str(csv), str(tmp_path / "cache"))
    spec = slots.SlotSpec.from_csv(str(csv))
    spec.save(str(tmp_path / "slot_map.json"))
    table = slots.TupleTable.from_csv(spec, str(csv))
    table.save(str(tmp_path / "slot_tuples.json"))
    assert 1 < len(table) <= 64 and len(table) < R.n_product(spec.sizes)
    cfg = {"batch_size": 8, "num_workers": 0, "num_labels": spec.total, "cache_dir": str(tmp_path / "cache"), "use_feature_cache": True,
           "save_path": str(tmp_path / "ckpt"), "device_metrics": True,
           "slots": {"map": str(tmp_path / "slot_map.json"), "tuples": str(tmp_path / "slot_tuples.json")}}
    sd = synth.synth_state_dict(spec.total, seed=0)
    torch.save(sd, str(tmp_path / "model.pt"))
    eargs = types.SimpleNamespace(test_csv=str(csv), label_map=None, model_path=str(tmp_path / "model.pt"))
    acc = ev.evaluate(eargs, cfg)
    out = tmp_path / "ckpt" / "evaluation_results"
    joint = json.load(open(out / "joint_metrics.json"))
    cons = json.load(open(out / "constrained_metrics.json"))
    assert joint["exact_match_accuracy"] == acc and (out / "classification_report_intents.txt").exists()
    # the reference's count, on the logits the same model gives for the same features
    from sir_amd.models.models import CNNAudioGRU
    from sir_amd.scripts.dataset import FSCIntentDataset
    ds = FSCIntentDataset(csv_path=str(csv), label_map_path=None, is_training=False, use_cache=True, cache_dir=str(tmp_path / "cache"),
                          slot_spec=spec)
    from sir_amd.scripts.train import collate_fn
    mel, lab = collate_fn([ds[i] for i in range(len(ds))])
    model = CNNAudioGRU(spec.total)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    with torch.no_grad():
        logits = model(mel.to(DEV)).cpu().numpy()
    labels = lab.numpy()
    ref_index, _, ref_logp, _, ref_mass, _ = R.decode_table(logits, spec.sizes, np.asarray(table.rows), 2, None)
    assert (ref_logp[:, 0] - ref_logp[:, 1] > 2 * R.SCORE_BOUND).all()                    # no decision of this split hangs on a rounding
    want = int((ref_index[:, 0] == table.encode(labels)).sum())
    assert cons["n"] == 16 and cons["n_tuples"] == len(table) and cons["exact_match"] == want and cons["exact_match_accuracy"] == want / 16
    assert abs(cons["mean_valid_mass"] - ref_mass.mean()) <= R.prob_bound(3)
    assert cons["exact_match_accuracy"] >= joint["exact_match_accuracy"] and joint["n"] == 16
    assert np.isfinite(cons["nll"]) and 0.0 <= cons["ece"] <= 1.0 and cons["calibration"]["n"] == 16
    ops.check_status()
