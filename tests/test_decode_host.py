"""Host: joint decoding of the slot heads without a GPU -- ``slots.TupleTable`` (validation, packing, encode, save / load), the
argument checks of ``slots.decode`` and of the result builders with every device call barred, the float64 reference
(tests/decode_ref.py) against torch, and the bounds of tests/test_decode_gpu.py against the float32 restatement."""
import json

import numpy as np
import pandas as pd
import pytest
import torch

import decode_ref as R
from sir_amd import _native, slots

FSC = (6, 14, 4)


@pytest.fixture
def no_device(monkeypatch):
    def barred(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_native, "require_hip", barred)
    monkeypatch.setattr(_native, "lib", barred)


def _spec():
    return slots.SlotSpec(["action", "object", "location"], [["a0", "a1"], ["o0", "o1", "o2"], ["l0", "l1"]])


def test_tuple_table_validation_errors_need_no_device(no_device):
    spec = _spec()
    for rows, what in (([], "1..4096"), ([(0, 0)], "labels for 3 slots"), ([(0, 3, 0)], "outside"), ([(2, 0, 0)], "outside"),
                       ([(0, 0, -1)], "outside"), ([(0, 0, 0), (1, 1, 1), (0, 0, 0)], "same tuple"), ([(0, 0, True)], "outside"),
                       ([(0, 0.0, 0)], "outside"), (5, "sequence")):
        with pytest.raises(ValueError, match=what):
            slots.TupleTable(spec, rows)
    with pytest.raises(ValueError, match="1..4096"):
        slots.TupleTable((64,), [(i % 64,) for i in range(4097)])
    with pytest.raises(ValueError, match="at most 4096"):
        slots.TupleTable.full((8,) * 8)
    with pytest.raises(ValueError, match="at most 4096"):
        slots.TupleTable.full((17, 16, 16))
    assert len(slots.TupleTable.full((16, 16, 16))) == 4096
    table = slots.TupleTable(spec, [(1, 2, 0), (0, 0, 1)])
    logits = torch.zeros(4, 7)
    for kw, what in ((dict(k=0), "k must"), (dict(k=9), "k must"), (dict(want_scores=True), "needs a table"),
                     (dict(table=[(0, 0, 0)]), "TupleTable"), (dict(table=slots.TupleTable.full((2, 3, 3))), "layout"),
                     (dict(table=table, inv_temperature=[1.0, -1.0, 1.0]), "positive"), (dict(inv_temperature=[1.0, 1.0]), "2 inverse")):
        with pytest.raises(ValueError, match=what):
            slots.decode(logits, spec, **kw)
    with pytest.raises(ValueError, match="columns"):
        slots.decode(torch.zeros(4, 8), spec, table=table)
    from sir_amd.scripts import classify_results
    for args in ((logits, spec, 3, None, None, table, "independent"), (logits, spec, 3, None, None, None, "best")):
        with pytest.raises(ValueError):
            classify_results.results_from_slot_logits(*args)
    with pytest.raises(ValueError, match="slot layout"):
        classify_results.results_of(logits, {}, None, None, None, table, "joint")
    from sir_amd.scripts import predict_frontend
    with pytest.raises(ValueError, match="slot layout"):
        predict_frontend.predict_many(None, [], {}, "cpu", decode="joint")


def test_packing_byte_order_and_zero_padding():
    table = slots.TupleTable(FSC, [(5, 13, 3), (0, 7, 2), (1, 0, 0)])
    assert table.packed.dtype == np.uint8 and table.packed.shape == (3, 8) and table.packed.flags["C_CONTIGUOUS"]
    assert table.packed.tolist() == [[5, 13, 3, 0, 0, 0, 0, 0], [0, 7, 2, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]]
    assert table.packed.view("<u8")[:, 0].tolist() == [5 + (13 << 8) + (3 << 16), (7 << 8) + (2 << 16), 1]     # slot g = byte g of the word
    assert table.index == {(5, 13, 3): 0, (0, 7, 2): 1, (1, 0, 0): 2} and table.rows[1] == (0, 7, 2) and len(table) == 3
    full = slots.TupleTable.full((2, 3))
    assert full.rows == ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2))                     # row t = mixed-radix number t
    assert np.array_equal(R.mixed_radix(np.asarray(full.rows), (2, 3)), np.arange(6))
    eight = slots.TupleTable((8,) * 8, [tuple(range(8))])
    assert eight.packed.tolist() == [list(range(8))]


def test_encode_unknown_and_ignored_tuples():
    table = slots.TupleTable(_spec(), [(1, 2, 0), (0, 0, 1)])
    labels = np.asarray([[0, 0, 1], [1, 2, 0], [1, 2, 1], [-100, 0, 1], [0, 0, -100], [0, 0, 1]])
    want = [1, 0, -100, -100, -100, 1]
    got = table.encode(labels)
    assert got.dtype == np.int64 and got.tolist() == want and table.encode(torch.from_numpy(labels)).tolist() == want
    assert table.encode(np.zeros((0, 3), dtype=np.int64)).shape == (0,)
    with pytest.raises(ValueError):
        table.encode(np.zeros((4, 2), dtype=np.int64))


def test_save_load_round_trip_and_dataframe_constructor(tmp_path):
    spec = _spec()
    frame = pd.DataFrame({"action": ["a1", "a0", "a1", "a0", "a9"], "object": ["o2", "o0", "o2", "o1", "o0"],
                          "location": ["l0", "l1", "l0", "l1", "l0"]})
    table = slots.TupleTable.from_dataframe(spec, frame)
    assert table.rows == ((0, 0, 1), (0, 1, 1), (1, 2, 0))                                   # distinct, sorted, the unknown row left out
    frame.to_csv(tmp_path / "d.csv", index=False)
    assert slots.TupleTable.from_csv(spec, str(tmp_path / "d.csv")) == table
    path = tmp_path / "slot_tuples.json"
    table.save(str(path))
    assert set(json.load(open(path))) == {"columns", "vocab", "tuples"}
    back = slots.TupleTable.load(str(path))
    assert back == table and back.spec == spec and np.array_equal(back.packed, table.packed)
    assert slots.TupleTable.load(str(path), spec) == table
    with pytest.raises(ValueError, match="layout"):
        slots.TupleTable.load(str(path), slots.SlotSpec.from_sizes((2, 3, 2)))
    spec.save(str(tmp_path / "slot_map.json"))                                                # slot_map.json keeps its format
    assert set(json.load(open(tmp_path / "slot_map.json"))) == {"columns", "vocab"}
    with pytest.raises(ValueError, match="not a tuple table"):
        slots.TupleTable.load(str(tmp_path / "slot_map.json"))
    assert table.names() == ["a0_o0", "a0_o1", "a1_o2"]
    assert slots.TupleTable(spec, [(0, 0, 0), (0, 0, 1)]).names() == ["a0_o0_l0", "a0_o0_l1"]


def test_reference_against_torch_float64():
    for sizes in ((6, 14, 4), (1, 63), (8,) * 8):
        x = R.case(sizes, 17)
        betas = R.betas_of(sizes)
        lp = R.log_softmax_slots(x, sizes, betas)
        for g, (a, c) in enumerate(zip(R.starts(sizes), sizes)):
            want = torch.log_softmax(torch.from_numpy(x[:, a:a + c]).double() * float(np.float32(betas[g])), dim=1).numpy()
            assert np.abs(lp[:, a:a + c] - want).max() <= 1e-11 * max(1.0, np.abs(want).max())
        rows = R.table_rows(sizes, 63)
        index, labels, logp, prob, mass, s = R.decode_table(x, sizes, rows, 8, betas)
        t = torch.from_numpy(s)
        top = torch.topk(t, 8, dim=1)
        assert np.allclose(logp, top.values.numpy(), rtol=0, atol=1e-9) and np.array_equal(labels, rows[index])
        assert np.allclose(prob, torch.softmax(t, dim=1).gather(1, torch.from_numpy(index)).numpy(), rtol=1e-9, atol=1e-300)
        assert np.allclose(mass, torch.logsumexp(t, dim=1).exp().numpy(), rtol=1e-9, atol=1e-300)
    # the order: descending score, an equal score by ascending row; padding past the table; a label outside its slot
    x = np.zeros((2, 24), dtype=np.float32)
    index, labels, logp, prob, mass, s = R.decode_table(x, FSC, R.table_rows(FSC, 2), 3)
    assert index.tolist() == [[0, 1, -1]] * 2 and np.isneginf(logp[:, 2]).all() and (prob[:, 2] == 0).all() and (labels[:, 2] == -1).all()
    assert np.allclose(prob[:, :2], 0.5) and np.allclose(mass, 2 / 336)
    index, _, _, prob, mass, s = R.decode_table(x, FSC, [(0, 14, 0), (1, 1, 1)], 2)
    assert index.tolist() == [[1, -1]] * 2 and np.isneginf(s[:, 0]).all() and np.allclose(prob[:, 0], 1.0) and np.allclose(mass, 1 / 336)
    x[1, 3] = np.nan
    out = R.decode_table(x, FSC, R.table_rows(FSC, 2), 3)
    assert (out[0][1] == -1).all() and np.isnan(out[2][1]).all() and np.isnan(out[4][1]) and np.isnan(out[5][1]).all() and out[0][0, 0] == 0


def test_enumeration_lazy_search_and_full_table_agree():
    for sizes in ((6, 14, 4), (31, 33), (4,) * 6):
        x = R.case(sizes, 17) if sizes in R.LAYOUTS else (np.random.default_rng(1).standard_normal((17, sum(sizes))) * 3).astype(np.float32)
        index, labels, logp, prob, s = R.decode_product(x, sizes, 8)
        assert np.array_equal(index, R.mixed_radix(labels, sizes)) and np.allclose(prob, np.exp(logp))
        full = slots.TupleTable.full(sizes)
        assert np.array_equal(np.asarray(full.rows), R.product_rows(sizes))
        t_index, _, t_logp, _, t_mass, _ = R.decode_table(x, sizes, np.asarray(full.rows), 8)
        assert np.array_equal(t_index, index) and np.array_equal(t_logp, logp) and np.allclose(t_mass, 1.0, rtol=0, atol=1e-12)
        lp = R.log_softmax_slots(x, sizes)
        for b in range(17):
            lazy = R.kbest_lazy(lp[b], sizes, 8)
            assert np.allclose([v[0] for v in lazy], logp[b], rtol=0, atol=1e-9) and [v[1] for v in lazy] == [tuple(r) for r in labels[b].tolist()]


def test_bounds_are_four_times_the_restatement_error():
    """SCORE_BOUND and PROB_BOUND of tests/decode_ref.py: the float32 restatement against float64 over every input of the GPU
    parity sweep, at 4 x margin (and no tighter than needed by more than a rounding-up)."""
    worst_s = worst_p = 0.0
    for sizes in R.LAYOUTS:
        for batch in R.BATCHES:
            x = R.case(sizes, batch)
            for n in R.table_sizes(sizes):
                rows = R.table_rows(sizes, n)
                assert len({tuple(r) for r in rows.tolist()}) == n                          # drawn without repetition
                for betas in (None, R.betas_of(sizes)):
                    es, ep = R.worst_restatement_errors(x, sizes, rows, betas)
                    worst_s, worst_p = max(worst_s, es), max(worst_p, ep)
    print(f"float32 restatement: worst score error {worst_s:.3e} (bound {R.SCORE_BOUND:.1e}), worst probability error {worst_p:.3e} "
          f"(bound {R.PROB_BOUND:.1e})")
    assert 4 * worst_s <= R.SCORE_BOUND <= 5 * worst_s and 4 * worst_p <= R.PROB_BOUND <= 5 * worst_p
    assert R.prob_bound(1) == R.PROB_BOUND and R.prob_bound(8) == max(3.2e-5, R.PROB_BOUND)
