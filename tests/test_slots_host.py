"""CPU: slot heads (include/sir_hip.h "slot heads", sir_amd/slots.py) -- the declared symbols and their binding, ``SlotSpec``,
the state layout arithmetic, host-side validation with the device barred, the float64 reference (tests/slots_ref.py) against
torch, and the conditions the GPU tests' inputs must meet."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pandas as pd
import pytest
import torch
import torch.nn.functional as F

import eval_ref
import slots_ref
from sir_amd import _native, metrics, slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sir_ce_loss_slots", "sir_classify_slots", "sir_eval_slots_state_bytes", "sir_eval_accumulate_slots"]


def _bar_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_native, "lib", no_device)
    monkeypatch.setattr(_native, "require_hip", no_device)
    monkeypatch.setattr(_native, "current_stream_ptr", no_device)


def _rows():
    return pd.DataFrame({"path": [f"{i}.wav" for i in range(5)],
                         "action": ["activate", "bring", "activate", "increase", "bring"],
                         "object": ["lights", "shoes", "music", "heat", "shoes"],
                         "location": ["kitchen", "bedroom", "none", "kitchen", "kitchen"]})


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_four_symbols_and_the_binding_carries_them():
    text = open(os.path.join(ROOT, "include", "sir_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _native.lib()
    for name in SYMBOLS:
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, f"{name} is not declared in sir_hip.h"
        n_args = len([a for a in m.group(2).split(",") if a.strip()])
        res, args = _native.SIGNATURES[name]
        assert len(args) == n_args, name
        assert res is (C.c_size_t if m.group(1) == "size_t" else C.c_int), name
        assert hasattr(lib, name)
    assert lib.sir_abi_version() == 1
    assert "bit-identical to sir_ce_loss_soft" in text and "slots_correct[9]" in text      # the contract sits in the header


def test_state_size_and_unpack_against_the_documented_layout():
    lib = _native.lib()
    for sizes, m in [((6, 14, 4), 15), ((1,), 1), ((31, 33), 64), ((8,) * 8, 10)]:
        arr = (C.c_int32 * len(sizes))(*sizes)
        joint = 2 + 9 + 1 + 3 * m + 1 + 64 * (m + 1)
        want = 8 * (sum(lib.sir_eval_state_bytes(c, m) // 8 for c in sizes) + joint)
        assert lib.sir_eval_slots_state_bytes(arr, len(sizes), m) == want == 8 * slots.state_words(sizes, m)
    arr = (C.c_int32 * 3)(6, 14, 4)
    assert lib.sir_eval_slots_state_bytes(arr, 3, 0) == 0 and lib.sir_eval_slots_state_bytes(arr, 3, 65) == 0
    assert lib.sir_eval_slots_state_bytes(arr, 0, 15) == 0 and lib.sir_eval_slots_state_bytes(None, 3, 15) == 0
    assert lib.sir_eval_slots_state_bytes((C.c_int32 * 9)(*([1] * 9)), 9, 15) == 0
    assert lib.sir_eval_slots_state_bytes((C.c_int32 * 2)(6, 0), 2, 15) == 0
    assert lib.sir_eval_slots_state_bytes((C.c_int32 * 2)(32, 33), 2, 15) == 0
    # unpack: every field filled with its own value at the documented offset
    sizes, m = (2, 3), 4
    words = np.zeros(slots.state_words(sizes, m), dtype=np.int64)
    o = metrics.state_words(2, m) + metrics.state_words(3, m)
    words[metrics.state_words(2, m) + 3 * 3] = 77                                        # slot 1: n behind its 3 x 3 confusion
    words[o], words[o + 1] = 11, 7
    words[o + 2: o + 11] = np.arange(9)
    words[o + 11: o + 12] = np.array([2.5]).view(np.int64)
    words[o + 12: o + 16] = [1, 2, 3, 5]
    words[o + 16: o + 20] = [0, 1, 2, 4]
    words[o + 20: o + 24] = np.array([0.1, 0.2, 0.3, 0.4]).view(np.int64)
    words[o + 24] = 9
    st = slots.unpack_state(words, sizes, m)
    j = st["joint"]
    assert st["slots"][1]["n"] == 77 and st["slots"][0]["n"] == 0 and len(st["slots"]) == 2
    assert (j["n"], j["exact_match"], j["n_excluded"], j["nll_sum"]) == (11, 7, 9, 2.5)
    assert j["slots_correct"].tolist() == list(range(9)) and j["bin_count"].tolist() == [1, 2, 3, 5]
    assert j["bin_correct"].tolist() == [0, 1, 2, 4] and j["bin_conf_sum"].tolist() == [0.1, 0.2, 0.3, 0.4]
    merged = slots.merge(st, st)
    assert merged["joint"]["n"] == 22 and merged["joint"]["nll_sum"] == 5.0 and merged["slots"][1]["n"] == 154
    with pytest.raises(ValueError):
        slots.unpack_state(words[:-1], sizes, m)
    with pytest.raises(ValueError, match="add up"):
        slots.joint_report(j)                                                            # 11 rows, bins hold 11, slots_correct 36


def test_c_entry_points_refuse_on_the_host():
    """NULL handle / layout errors come back as SIR_EINVAL without a device (every check precedes the first launch)."""
    lib = _native.lib()
    buf = C.create_string_buffer(64)
    one = C.addressof(buf)
    sizes = (C.c_int32 * 3)(6, 14, 4)
    assert lib.sir_ce_loss_slots(None, one, one, None, None, 0.0, sizes, None, 3, 1, 24, one, None, None, 1.0, None) == _native.SIR_EINVAL
    assert lib.sir_classify_slots(None, one, 1, 24, sizes, 3, None, 1, None, one, one, None, None) == _native.SIR_EINVAL
    assert lib.sir_eval_accumulate_slots(None, one, one, 1, 24, sizes, 3, None, 15, one, 1 << 20, None) == _native.SIR_EINVAL


# ---- SlotSpec -----------------------------------------------------------------------------------------------------------------
def test_slot_spec_round_trip(tmp_path, caplog):
    csv = tmp_path / "train_data.csv"
    _rows().to_csv(csv, index=False)
    spec = slots.SlotSpec.from_csv(str(csv))
    assert spec.columns == ("action", "object", "location")
    assert spec.vocab == (("activate", "bring", "increase"), ("heat", "lights", "music", "shoes"), ("bedroom", "kitchen", "none"))
    assert spec.sizes == (3, 4, 3) and spec.starts == (0, 3, 7) and spec.total == 10 and spec.n_slots == 3
    spec.save(str(tmp_path / "slot_map.json"))
    assert json.load(open(tmp_path / "slot_map.json"))["columns"] == ["action", "object", "location"]
    back = slots.SlotSpec.load(str(tmp_path / "slot_map.json"))
    assert back == spec
    enc = back.encode(_rows())
    assert enc.dtype == np.int64 and enc.tolist() == [[0, 1, 1], [1, 3, 0], [0, 2, 2], [2, 0, 1], [1, 3, 1]]
    dec = back.decode(enc[1])
    assert dec == {"action": "bring", "object": "shoes", "location": "bedroom"}
    assert back.reference_label(dec) == "bring_shoes"                                   # the reference's own join: location dropped
    # the two utterances the reference cannot tell apart
    assert enc[1].tolist() != enc[4].tolist() and back.reference_label(back.decode(enc[4])) == "bring_shoes"
    other = _rows()
    other.loc[0, "object"] = "newspaper"
    other.loc[2, "object"] = "socks"
    with caplog.at_level("WARNING"):
        enc2 = back.encode(other)
        back.encode(other)
    assert enc2[0].tolist() == [0, -100, 1] and enc2[2].tolist() == [0, -100, 2] and (enc2[[1, 3, 4]] == enc[[1, 3, 4]]).all()
    assert sum("unknown value" in r.message for r in caplog.records) == 1               # logged once per column
    assert back.decode([0, -100, 1])["object"] == "Unknown"
    two = slots.SlotSpec(["action", "location"], [["a", "b"], ["x"]])
    assert two.reference_label({"action": "a", "location": "x"}) is None
    assert slots.SlotSpec.from_sizes((6, 14, 4)).sizes == (6, 14, 4)
    for bad in ([], [1] * 9, [0, 3], [32, 33], [2.5], [True]):
        with pytest.raises(ValueError):
            slots.check_sizes(bad)
    with pytest.raises(ValueError):
        slots.SlotSpec(["a", "a"], [["x"], ["y"]])
    with pytest.raises(ValueError):
        slots.SlotSpec(["a"], [["x", "x"]])
    with pytest.raises(ValueError):
        slots.SlotSpec.from_csv(str(csv), columns=("action", "room"))


# ---- validation with the device barred ----------------------------------------------------------------------------------------
def test_every_validation_error_is_raised_before_any_device_call(monkeypatch):
    _bar_device(monkeypatch)
    spec = slots.SlotSpec.from_sizes((6, 14, 4))
    x = torch.zeros(5, 24)
    y = torch.zeros(5, 3, dtype=torch.int64)
    lam = torch.ones(5)
    ce = slots.slot_cross_entropy
    for call in (lambda: ce(torch.zeros(5, 23), y, spec), lambda: ce(x.double(), y, spec), lambda: ce(x, y[:, :2], spec),
                 lambda: ce(x, y.int(), spec), lambda: ce(x, y, spec, weights=[1.0, 2.0]),
                 lambda: ce(x, y, spec, weights=[1.0, float("nan"), 1.0]), lambda: ce(x, y, spec, weights=[1.0, -1.0, 1.0]),
                 lambda: ce(x, y, spec, weights=[1.0, float("inf"), 1.0]), lambda: ce(x, y, spec, lam=lam),
                 lambda: ce(x, y, spec, labels_b=y[:4]), lambda: ce(x, y, spec, labels_b=y, lam=lam[:4]),
                 lambda: ce(x, y, spec, label_smoothing=1.0), lambda: ce(x, y, spec, label_smoothing=-0.1),
                 lambda: ce(x, y, (6, 14, 5)), lambda: ce(x, y, (6, 0, 18)),
                 lambda: slots.SlotLoss(spec, weights=[1.0]), lambda: slots.SlotLoss(spec, label_smoothing=2.0),
                 lambda: slots.classify(x, spec, k=0), lambda: slots.classify(x, spec, k=9), lambda: slots.classify(x, spec, k=True),
                 lambda: slots.classify(x[:, :20], spec), lambda: slots.classify(x, spec, inv_temperature=[1.0, 2.0]),
                 lambda: slots.classify(x, spec, inv_temperature=0.0), lambda: slots.classify(x, spec, inv_temperature=[1.0, -2.0, 1.0]),
                 lambda: slots.classify(x, spec, inv_temperature=torch.ones(2)),
                 lambda: slots.SlotEvalAccumulator(spec, n_bins=0), lambda: slots.SlotEvalAccumulator(spec, n_bins=65),
                 lambda: slots.SlotEvalAccumulator(spec, inv_temperature=[1.0]),
                 lambda: slots.SlotEvalAccumulator(spec).update(x, y[:, :2]), lambda: slots.SlotEvalAccumulator(spec).update(x[:, :5], y),
                 lambda: slots.fit_slot_temperatures(x, y, spec, iters=-1), lambda: slots.fit_slot_temperatures(x, y[:, :1], spec)):
        with pytest.raises(ValueError):
            call()
    # ... and valid arguments do go on to the device, which is barred here
    for call in (lambda: ce(x, y, spec), lambda: slots.classify(x, spec), lambda: slots.SlotEvalAccumulator(spec).update(x, y)):
        with pytest.raises(AssertionError, match="device call"):
            call()
    # an accumulator that has seen nothing reports an empty state without a device
    res = slots.SlotEvalAccumulator(spec).result()
    assert res["joint"]["n"] == 0 and np.isnan(res["joint"]["exact_match_accuracy"]) and set(res["slots"]) == set(spec.columns)


def test_results_route_validates_before_any_device_call(monkeypatch):
    from sir_amd.scripts import classify_results, predict_frontend
    _bar_device(monkeypatch)
    spec = slots.SlotSpec.from_sizes((6, 14, 4))
    assert classify_results.slot_inv_temperature_of(None, 3) is None
    assert classify_results.slot_inv_temperature_of(2.0, 3) == [0.5, 0.5, 0.5]
    assert classify_results.slot_inv_temperature_of([1.0, 2.0, 4.0], 3) == [1.0, 0.5, 0.25]
    for bad in ([1.0, 2.0], 0.0, [1.0, -1.0, 1.0]):
        with pytest.raises(ValueError):
            classify_results.slot_inv_temperature_of(bad, 3)
        with pytest.raises(ValueError):
            predict_frontend.predict_many(None, ["a.wav"], {}, "cpu", slots=spec, temperature=bad)
    with pytest.raises(ValueError):
        classify_results.results_from_slot_logits(torch.zeros(2, 24), spec, k=9)


def test_train_refuses_a_slot_layout_that_is_not_num_labels_before_any_device_call(tmp_path, monkeypatch):
    from sir_amd.scripts import train as tr
    _bar_device(monkeypatch)
    csv = tmp_path / "train_data.csv"
    _rows().to_csv(csv, index=False)
    args = types.SimpleNamespace(train_csv=str(csv), val_csv=str(csv), label_map=None)
    cfg = {"batch_size": 4, "num_labels": 31, "slots": {"columns": ["action", "object", "location"]}}
    with pytest.raises(ValueError, match="num_labels is 31"):
        tr.train(args, cfg)
    slots.SlotSpec.from_csv(str(csv)).save(str(tmp_path / "slot_map.json"))
    with pytest.raises(ValueError, match="num_labels is 24"):
        tr.train(args, dict(cfg, num_labels=24, slots={"map": str(tmp_path / "slot_map.json")}))
    with pytest.raises(ValueError, match="slot weights"):
        tr.train(args, dict(cfg, num_labels=10, slots={"weights": [1.0, 2.0]}))
    with pytest.raises(ValueError, match="unknown keys"):
        tr.train(args, dict(cfg, num_labels=10, slots={"colums": ["action"]}))
    with pytest.raises(AssertionError, match="device call"):                             # a consistent layout goes on to the device
        tr.train(args, dict(cfg, num_labels=10))
    opts = tr.slot_options(dict(cfg, num_labels=10, slots={"weights": [1, 2, 0]}), str(csv))
    assert opts["spec"].sizes == (3, 4, 3) and opts["weights"] == [1.0, 2.0, 0.0]
    assert tr.slot_options({"num_labels": 31}) is None


def test_datasets_hand_out_slot_labels(tmp_path, monkeypatch):
    from sir_amd.scripts.dataset import FSCIntentDataset
    from sir_amd.scripts.train import collate_fn
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)                       # no prefetch in the constructor
    csv = tmp_path / "train_data.csv"
    rows = _rows()
    rows.to_csv(csv, index=False)
    spec = slots.SlotSpec.from_csv(str(csv))
    cache = tmp_path / "cache"
    cache.mkdir()
    torch.save({p: {"features": torch.ones(64, 7), "label": "x"} for p in rows["path"]}, str(cache / "train_data_features.pt"))
    ds = FSCIntentDataset(str(csv), None, is_training=False, cache_dir=str(cache), slot_spec=spec)
    mel, label = ds[1]
    assert label.dtype == torch.int64 and label.tolist() == [1, 3, 0] and mel.shape == (64, 200)
    mels, labels = collate_fn([ds[i] for i in range(5)])
    assert mels.shape == (5, 64, 200) and labels.dtype == torch.int64 and labels.tolist() == spec.encode(rows).tolist()


# ---- the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(6, 14, 4), (31, 33), (1, 63), (2, 2, 2, 2, 2, 2, 2, 50)])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_reference_loss_agrees_with_torch_float64(sizes, eps):
    logits, ya, yb, lam = slots_ref.case(sizes, 17, second=True)
    w = slots_ref.weights_of(sizes)
    lg = logits.double().requires_grad_(True)
    want = sum(w[g] * F.cross_entropy(lg[:, a:b], ya[:, g], label_smoothing=eps) for g, (a, b) in enumerate(slots_ref.segments(sizes)))
    want.backward()
    loss, slot_losses, d = slots_ref.soft_ce_slots(logits, ya, sizes, w, eps=eps)
    assert abs(loss.item() - want.item()) <= 1e-12 * max(1.0, abs(want.item()))
    assert (d - lg.grad).abs().max().item() <= 1e-14
    assert (d[2, :sizes[0]] == 0).all() and (d[16, -sizes[-1]:] == 0).all()               # the two ignored (row, slot) pairs
    # mixup's two label sets: lam per row, for all slots of the row
    yb_ok = yb.clone()
    yb_ok[2, 0] = 0
    per_row = sum(w[g] * (lam.double() * F.cross_entropy(logits.double()[:, a:b], ya[:, g], label_smoothing=eps, reduction="none")
                          + (1 - lam.double()) * F.cross_entropy(logits.double()[:, a:b], torch.where(ya[:, g] == -100, ya[:, g], yb_ok[:, g]),
                                                                label_smoothing=eps, reduction="none")).sum()
                  / (ya[:, g] != -100).sum() for g, (a, b) in enumerate(slots_ref.segments(sizes)))
    mixed = slots_ref.soft_ce_slots(logits, ya, sizes, w, yb, lam, eps)[0]
    assert abs(mixed.item() - per_row.item()) <= 1e-12 * max(1.0, abs(per_row.item()))


def test_reference_classification_and_joint_block():
    sizes = (2, 3, 1)
    logits = np.array([[2.0, 0.0, 1.0, 3.0, 0.0, 5.0],
                       [0.0, 1.0, 0.0, 0.0, 4.0, -2.0],
                       [1.0, 2.0, np.nan, 0.0, 0.0, 0.0],
                       [0.5, 0.5, 1.0, 1.0, 0.0, 0.0]])
    labels = np.array([[0, 1, 0], [0, 2, 0], [1, 0, 0], [0, -100, 0]])
    probs, idx, top, joint = slots_ref.classify_slots(logits, sizes, 2)
    p0 = np.exp([2.0, 0.0]) / np.exp([2.0, 0.0]).sum()
    p1 = np.exp([1.0, 3.0, 0.0]) / np.exp([1.0, 3.0, 0.0]).sum()
    assert np.allclose(probs[0], np.concatenate([p0, p1, [1.0]]), rtol=1e-15)
    assert idx[0].tolist() == [[0, 1], [1, 0], [0, -1]] and top[0, 2].tolist() == [1.0, 0.0]
    assert np.isclose(joint[0], p0[0] * p1[1], rtol=1e-15)
    assert idx[2, 1].tolist() == [-1, -1] and np.isnan(top[2, 1]).all() and np.isnan(joint[2]) and idx[2, 0].tolist() == [1, 0]
    assert idx[3, 0].tolist() == [0, 1] and idx[3, 1].tolist() == [0, 1]                    # ties: the lower index first
    st = slots_ref.eval_accumulate_slots(slots_ref.empty_state(sizes, 4), logits, labels, sizes, 4)
    j = st["joint"]
    assert (j["n"], j["n_excluded"], j["exact_match"]) == (2, 2, 1)                       # rows 2 (NaN) and 3 (-100) are left out
    assert j["slots_correct"].tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0]                     # row 1: slot 0 wrong (predicts 1)
    assert np.isclose(j["nll_sum"], -np.log(p0[0]) - np.log(p1[1]) - np.log(probs[1, 0]) - np.log(probs[1, 4]), rtol=1e-14)
    assert j["bin_count"].sum() == 2 and j["bin_correct"].sum() == 1 and np.isclose(j["bin_conf_sum"].sum(), joint[0] + joint[1])
    assert [s["n"] for s in st["slots"]] == [4, 2, 4] and st["slots"][1]["n_ignored"] == 1 and st["slots"][1]["n_nonfinite"] == 1
    # through the library's own host code: unpacked states -> reports
    rep = slots.joint_report(j)
    assert rep["exact_match_accuracy"] == 0.5 and rep["n_excluded"] == 2 and np.isclose(rep["nll"], j["nll_sum"] / 2)
    assert metrics.report_from_state(st["slots"][0])["accuracy"] == 0.75
    assert json.dumps(slots.joint_json(rep))


@pytest.mark.parametrize("sizes", slots_ref.LAYOUTS, ids=lambda s: "x".join(map(str, s)) if len(set(s)) > 1 else f"{s[0]}x{len(s)}")
@pytest.mark.parametrize("batch", slots_ref.BATCHES)
def test_generated_inputs_meet_the_conditions_for_every_row(sizes, batch):
    """In float64, for ALL rows, with beta = 1 and with the tests' per-slot betas: the top-2 logit gap inside each slot is above
    1e-4 and the joint confidence lies at least 1e-4 / n_bins from every (interior) bin edge."""
    logits, ya, _, _ = slots_ref.case(sizes, batch)
    assert logits.shape == (batch, sum(sizes)) and ya.shape == (batch, len(sizes))
    for betas in (None, slots_ref.betas_of(sizes)):
        gap, edge = slots_ref.condition_margins(logits, ya, sizes, slots_ref.N_BINS, betas)
        assert gap.shape == (batch,) and (gap > slots_ref.GAP_MIN).all(), gap.min()
        assert (edge >= slots_ref.EDGE_MIN).all(), edge.min()
    logits2, ya2, yb, lam = slots_ref.case(sizes, batch, second=True)                     # the same logits and first labels
    assert torch.equal(logits, logits2) and torch.equal(ya, ya2) and yb.shape == ya.shape and lam.shape == (batch,)
