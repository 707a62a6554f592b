"""CPU: the float64 reference of the prototype head checks itself, the fp32 restatement's measured error sits well inside the
derived bounds, and the host half of ``sir_amd.prototypes`` (names, limits, the bank file, the callers' keyword checks)."""
import numpy as np
import pytest
import torch

import proto_ref
from proto_ref import SIM_BOUND, prob_bound
from sir_amd import _native
from sir_amd.prototypes import MAX_PROTOTYPES, PrototypeBank
from sir_amd.scripts import classify_results


def _rows(n, seed, dim=proto_ref.DIM):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((n, dim)).astype(np.float32)


def _unit32(x):
    return proto_ref.unit_rows(x)[0].astype(np.float32)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_unit_rows_and_the_rows_that_are_skipped():
    x = _rows(6, 1)
    x[1, 7] = np.nan
    x[2, 500] = np.inf
    x[3] = 0.0
    x[4] *= np.float32(1e-30)
    u, ok = proto_ref.unit_rows(x)
    assert ok.tolist() == [True, False, False, False, True, True]
    assert np.allclose(np.linalg.norm(u[ok], axis=1), 1.0, atol=1e-15) and not u[~ok].any()
    # a row at 1e-30 has the direction of the unscaled row: the norm never leaves double
    assert np.abs(u[4] - proto_ref.unit_rows(_rows(6, 1)[4:5] * np.float32(1e-30))[0][0]).max() == 0.0
    assert np.abs(u[4] - proto_ref.unit_rows(_rows(6, 1)[4:5])[0][0]).max() < 1e-6          # (fp32 scaling rounds the inputs)


def test_accumulate_is_a_sum_of_unit_rows_and_finalize_normalises():
    x = _rows(40, 2)
    labels = np.arange(40) % 5
    labels[3], labels[11] = -1, 5
    total, count = np.zeros((5, 512)), np.zeros((5,), np.int64)
    assert proto_ref.accumulate(total, count, x, labels) == 2
    u, _ = proto_ref.unit_rows(x)
    keep = (labels >= 0) & (labels < 5)
    for c in range(5):
        assert np.allclose(total[c], u[keep & (labels == c)].sum(axis=0), rtol=0, atol=1e-13)
    assert count.tolist() == [8, 7, 8, 7, 8]
    # the same rows in two calls: the same sequential chains, the same bits
    t2, c2 = np.zeros((5, 512)), np.zeros((5,), np.int64)
    proto_ref.accumulate(t2, c2, x[:17], labels[:17])
    proto_ref.accumulate(t2, c2, x[17:], labels[17:])
    assert np.array_equal(t2, total) and np.array_equal(c2, count)
    count[2] = 0
    protos, live = proto_ref.finalize(total, count)
    assert live.tolist() == [1, 1, 0, 1, 1] and not protos[2].any()
    assert np.allclose(np.linalg.norm(protos[live == 1].astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_score_reference_ranks_max_over_exemplars_and_breaks_ties_by_class():
    protos = _unit32(_rows(6, 3))
    protos[4] = protos[1]                                        # two identical prototypes in classes 0 and 2
    emb = _rows(3, 4)
    emb[2] = protos[1] * 3.0
    pclass = np.array([1, 2, 1, 3, 0, 7], np.int32)              # (prototype 5: a class outside the call's, takes no part)
    live = np.array([1, 1, 1, 0, 1, 1], np.uint8)
    out = proto_ref.score(emb, protos, live, pclass, n_classes=5, scale=16.0)
    assert out["present"].tolist() == [True, True, True, False, False]
    sims = proto_ref.unit_rows(emb)[0] @ protos.astype(np.float64).T
    assert np.array_equal(out["s"][:, 1], np.maximum(sims[:, 0], sims[:, 2]))
    assert out["order"][2].tolist()[:2] == [0, 2]                # equal scores: the lower class first
    assert np.allclose(out["prob"].sum(axis=1), 1.0) and not out["prob"][:, 3:].any()
    assert proto_ref.check_ranking(out["s"][2], [0, 2, 1, -1, -1], 5) is None
    assert proto_ref.check_ranking(out["s"][2], [2, 0, 1, -1, -1], 5) is None       # a tie inside 2 * SIM_BOUND may go either way
    assert "not -1" in proto_ref.check_ranking(out["s"][2], [0, 2, 1, 1, -1], 5)
    assert "distinct" in proto_ref.check_ranking(out["s"][2], [0, 0, 1, -1, -1], 5)
    assert proto_ref.check_ranking(out["s"][2], [1, 0, 2, -1, -1], 5) is not None


def test_fp32_restatement_sits_inside_the_bounds_with_room():
    """The measured error of the kernel's arithmetic (restated in numpy fp32, without the fma: a little worse) against float64 on
    the inputs the GPU tests use.  If this came near the bounds, the derivation would be wrong, not the tolerance."""
    worst_sim, worst_prob = 0.0, 0.0
    for bsz, n_protos, seed in ((17, 65, 10), (17, 4096, 11), (257, 65, 12)):
        emb, protos = _rows(bsz, seed), _unit32(_rows(n_protos, seed + 100))
        ref = proto_ref.score(emb, protos)
        got = proto_ref.sims_f32(emb, protos).astype(np.float64)
        err = np.abs(got - ref["sims"]).max()
        worst_sim = max(worst_sim, err)
        for scale in (1.0, 16.0, 64.0):
            p_ref = proto_ref.score(emb, protos, scale=scale)["prob"]
            z = scale * (got - got.max(axis=1, keepdims=True))
            p = (np.exp(z.astype(np.float32)) / np.exp(z.astype(np.float32)).sum(axis=1, keepdims=True, dtype=np.float64))
            ratio = (np.abs(p - p_ref) / prob_bound(p_ref, scale)).max()
            worst_prob = max(worst_prob, ratio)
    print(f"fp32 restatement: max |sim error| {worst_sim:.3e} (SIM_BOUND {SIM_BOUND:.3e}), "
          f"max probability error / prob_bound {worst_prob:.3f}")
    assert worst_sim <= SIM_BOUND / 4
    assert worst_prob <= 0.25


# ---- the bank on the host --------------------------------------------------------------------------------------------------
def test_names_and_limits():
    bank = PrototypeBank(["lights_on", "lights_off"])
    assert bank.names == ["lights_on", "lights_off"] and bank.n_rows == 2 and not bank.exemplars
    with pytest.raises(ValueError, match="twice"):
        PrototypeBank(["a", "a"])
    with pytest.raises(ValueError, match="non-empty string"):
        PrototypeBank([""])
    assert bank._resolve_labels(["lights_off", "volume_up", "lights_on", "volume_up"], 4) == [1, 2, 0, 2]
    assert bank.names[2] == "volume_up"
    assert bank._resolve_labels([0, -1, 7], 3) == [0, -1, 7]
    assert bank._resolve_labels(torch.tensor([2, 1]), 2) == [2, 1]
    with pytest.raises(ValueError, match="labels for"):
        bank._resolve_labels(["lights_on"], 2)
    with pytest.raises(ValueError, match="all names or all integers"):
        bank._resolve_labels(["lights_on", 1], 2)
    many = [f"intent_{i}" for i in range(MAX_PROTOTYPES)]
    full = PrototypeBank(many)
    assert len(full.names) == MAX_PROTOTYPES
    with pytest.raises(_native.SirError, match="at most 4096"):
        PrototypeBank(many + ["one_more"])
    with pytest.raises(_native.SirError, match="at most 4096"):
        full._resolve_labels(["intent_0", "one_more"], 2)
    assert len(full.names) == MAX_PROTOTYPES                     # a refused call extends nothing
    with pytest.raises(KeyError):
        bank.remove("never_seen")


def test_enroll_and_score_have_no_cpu_path():
    bank = PrototypeBank(["a", "b"])
    with pytest.raises(_native.SirError):
        bank.enroll(torch.zeros(2, 512), ["a", "b"])
    with pytest.raises(_native.SirError):
        bank.score(torch.zeros(2, 512))
    with pytest.raises(_native.SirError, match="empty"):
        PrototypeBank().prototypes()


@pytest.mark.parametrize("exemplars", [False, True])
def test_bank_file_round_trip(tmp_path, exemplars):
    names = ["lights_on", "lights_off", "größer"]
    bank = PrototypeBank(names, exemplars=exemplars)
    rows = 5 if exemplars else 3
    if exemplars:
        bank._row_class = [0, 2, 2, 1, 0]
    rng = np.random.Generator(np.random.PCG64(5))
    bank._host = {"sum": rng.standard_normal((rows, 512)), "count": np.arange(rows, dtype=np.int64), "skipped": 3}
    path = str(tmp_path / "bank.npz")
    bank.save(path)
    with np.load(path, allow_pickle=False) as z:                 # data only: four arrays (five for an exemplar bank)
        assert set(z.files) == {"sum", "count", "skipped", "names"} | ({"row_class"} if exemplars else set())
        assert z["sum"].dtype == np.float64 and z["count"].dtype == np.int64
    back = PrototypeBank.load(path)
    assert back.names == names and back.exemplars == exemplars and back._row_class == bank._row_class
    a, b = bank.state_arrays(), back.state_arrays()
    assert np.array_equal(a["sum"], b["sum"]) and np.array_equal(a["count"], b["count"]) and a["skipped"] == b["skipped"] == 3
    np.savez(str(tmp_path / "bad.npz"), sum=np.zeros((2, 512)), count=np.zeros((2,), np.int64), skipped=np.int64(0),
             names=np.asarray(names))
    with pytest.raises(ValueError, match="bank file"):
        PrototypeBank.load(str(tmp_path / "bad.npz"))


def test_keyword_checks_are_raised_before_any_device_call():
    from sir_amd import slots
    from sir_amd.scripts import predict_frontend
    from sir_amd.scripts.testing import IntentRecognizer
    bank = PrototypeBank(["a"])
    spec = slots.SlotSpec(["action", "object"], [["on", "off"], ["lights", "heat"]])
    with pytest.raises(ValueError, match="two different heads"):
        classify_results.check_prototypes(bank, None, slots=spec)
    with pytest.raises(ValueError, match="needs prototypes="):
        classify_results.check_prototypes(None, 0.5)
    with pytest.raises(ValueError, match="fc head"):
        classify_results.check_prototypes(bank, 0.5, temperature=2.0)
    with pytest.raises(ValueError, match="fc head"):
        classify_results.check_prototypes(bank, None, min_confidence=0.5)
    classify_results.check_prototypes(bank, 0.5)
    classify_results.check_prototypes(None, None, slots=spec, temperature=2.0, min_confidence=0.1)
    # the callers raise (they log and return None only for what goes wrong while scoring)
    with pytest.raises(ValueError, match="two different heads"):
        predict_frontend.predict_many(None, ["x.wav"], {}, "cuda", prototypes=bank, slots=spec)
    with pytest.raises(ValueError, match="needs prototypes="):
        predict_frontend.predict_many(None, ["x.wav"], {}, "cuda", min_similarity=0.3)
    reco = IntentRecognizer.__new__(IntentRecognizer)
    with pytest.raises(ValueError, match="two different heads"):
        reco.recognize_recordings([], prototypes=bank, slots=spec)
    with pytest.raises(ValueError, match="two different heads"):
        reco.open_streams(1, prototypes=bank, slots=spec)


_TWO_HEADS = "prototypes= and slots= are two different heads: pass one of them"
_FC_HEAD = "temperature= and min_confidence= belong to the fc head: with prototypes= use the bank's scale and min_similarity="
_NEEDS_ROUTE = "temperature= and min_confidence= need on_device=True (the per-row host route knows neither)"
# (keywords, the whole message); "bank" / "spec" / "table" stand for the objects the test builds
_REFUSALS = [
    (dict(prototypes="bank", slots="spec"), _TWO_HEADS),
    (dict(min_similarity=0.3), "min_similarity= needs prototypes= (a sir_amd.prototypes.PrototypeBank)"),
    (dict(prototypes="bank", temperature=2.0), _FC_HEAD),
    (dict(prototypes="bank", min_confidence=0.5), _FC_HEAD),
    (dict(temperature=2.0), _NEEDS_ROUTE),
    (dict(min_confidence=0.5), _NEEDS_ROUTE),
    (dict(decode="joint"), 'tuples= and decode="joint" need a slot layout (slots=)'),
    (dict(slots="spec", tuples="table"), 'a tuple table constrains joint decoding: pass decode="joint" with it'),
    (dict(slots="spec", decode="best"), 'decode must be "independent" or "joint", got \'best\''),
    (dict(slots="spec", temperature=[1.0, 2.0, 4.0]), "3 temperatures for 2 slots"),
    (dict(slots="spec", temperature=[1.0, 0.0]), "temperature must be a positive finite number, got 0.0"),
    (dict(prototypes="bank", slots="spec", temperature=2.0), _TWO_HEADS),
]


@pytest.mark.parametrize("keywords, message", _REFUSALS, ids=[" ".join(k) for k, _ in _REFUSALS[:-1]] + ["two rules broken"])
def test_every_caller_refuses_a_wrong_result_route_with_the_same_message(keywords, message, monkeypatch):
    from sir_amd import slots
    from sir_amd.scripts import predict_frontend
    from sir_amd.scripts.testing import IntentRecognizer

    def no_device(*a, **k):
        raise AssertionError("a device call before the keyword checks")

    for name in ("lib", "require_hip", "current_stream_ptr"):
        monkeypatch.setattr(_native, name, no_device)
    spec = slots.SlotSpec(["action", "object"], [["on", "off"], ["lights", "heat"]])
    objects = {"bank": PrototypeBank(["a"]), "spec": spec, "table": slots.TupleTable(spec, [(0, 0), (1, 1)])}
    kw = {k: objects.get(v, v) if isinstance(v, str) else v for k, v in keywords.items()}
    reco = IntentRecognizer.__new__(IntentRecognizer)
    callers = {"ResultOptions": lambda: classify_results.ResultOptions(**kw),
               "predict_many": lambda: predict_frontend.predict_many(None, ["x.wav"], {}, "cuda", **kw),
               "recognize_recordings": lambda: reco.recognize_recordings([], **kw),
               "open_streams": lambda: reco.open_streams(1, **kw)}
    for name, call in callers.items():
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == message, name
