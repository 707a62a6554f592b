"""CPU: the float64 reference of the classification / evaluation calls (tests/eval_ref.py) against sklearn and torch, the
host half of sir_amd.metrics (report_from_state, merge, format_report) and the argument checks that need no GPU."""
import numpy as np
import pytest
import torch

import eval_ref
from sir_amd import _native, metrics


def _random_predictions(n=500, c=7, seed=0):
    """labels and predictions over c classes; class 2 never occurs as a label, class 5 is never predicted."""
    rng = np.random.default_rng(seed)
    y = rng.choice([0, 1, 3, 4, 5, 6], size=n)
    p = np.where(rng.random(n) < 0.6, y, rng.choice([0, 1, 2, 3, 4, 6], size=n))
    p = np.where(p == 5, 2, p)
    assert 2 not in y and 5 not in p and 2 in p and 5 in y
    return y, p, c


def _assert_reports_equal(got, want):
    assert list(got) == list(want)
    for k, v in want.items():
        if isinstance(v, dict):
            assert list(got[k]) == list(v), k
            for kk, vv in v.items():
                assert got[k][kk] == pytest.approx(vv, rel=1e-14, abs=0), (k, kk)
        else:
            assert got[k] == pytest.approx(v, rel=1e-14, abs=0), k


def test_reference_confusion_and_report_match_sklearn():
    from sklearn.metrics import classification_report, confusion_matrix
    y, p, c = _random_predictions()
    cm, rep = eval_ref.confusion_and_report(y, p, c)
    assert np.array_equal(cm, confusion_matrix(y, p, labels=list(range(c))))
    want = classification_report(y, p, labels=list(range(c)), output_dict=True, zero_division=0)
    _assert_reports_equal(rep, want)
    assert rep["2"]["support"] == 0 and rep["5"]["precision"] == 0.0


def test_report_text_and_label_subset_match_sklearn():
    """evaluate.py reports the label map's classes of a wider head: predictions outside them turn `accuracy` into `micro avg`."""
    from sklearn.metrics import classification_report
    y, p, c = _random_predictions(seed=3)
    cm, _ = eval_ref.confusion_and_report(y, p, c)
    names = [f"intent_{i}_{'x' * i}" for i in range(c)]
    for labels in (list(range(c)), [0, 1, 3, 4]):
        tn = [names[i] for i in labels]
        want_dict = classification_report(y, p, labels=labels, target_names=tn, output_dict=True, zero_division=0)
        want_text = classification_report(y, p, labels=labels, target_names=tn, zero_division=0)
        got = metrics.classification_from_confusion(cm, tn, labels=labels)
        _assert_reports_equal(got, want_dict)
        assert metrics.format_report(got) == want_text
        assert ("micro avg" in got) == (len(labels) < c)


def test_reference_eval_state_matches_sklearn_on_logits():
    from sklearn.metrics import confusion_matrix, top_k_accuracy_score
    rng = np.random.default_rng(5)
    logits = rng.normal(size=(300, 6)).astype(np.float32) * 2
    labels = rng.integers(0, 6, size=300)
    st = eval_ref.eval_accumulate(eval_ref.empty_state(6, 10), logits, labels, 10)
    assert np.array_equal(st["confusion"], confusion_matrix(labels, logits.argmax(1), labels=list(range(6))))
    for k in (1, 3, 5):
        assert st["topk_correct"][k - 1] == round(top_k_accuracy_score(labels, logits, k=k, labels=list(range(6))) * 300)
    assert st["topk_correct"][5] == st["topk_correct"][7] == 300          # min(j + 1, C) = C from j = 5 on
    want_nll = torch.nn.functional.cross_entropy(torch.tensor(logits, dtype=torch.float64), torch.tensor(labels), reduction="sum")
    assert st["nll_sum"] == pytest.approx(float(want_nll), rel=1e-12)
    assert st["bin_count"].sum() == st["n"] == 300 and st["bin_correct"].sum() == np.trace(st["confusion"])


def test_reference_topk_matches_torch():
    rng = np.random.default_rng(1)
    for c, k in ((2, 1), (31, 3), (64, 8)):
        logits = rng.normal(size=(97, c)).astype(np.float32)
        for beta in (None, 0.5, 3.0):
            probs, idx, top = eval_ref.classify(logits, k, beta)
            scaled = torch.tensor(logits, dtype=torch.float64) * (1.0 if beta is None else beta)
            want = torch.softmax(scaled, dim=1)
            tv, ti = torch.topk(want, k, dim=1)
            assert np.array_equal(idx, ti.numpy())
            assert np.allclose(top, tv.numpy(), rtol=1e-13, atol=0) and np.allclose(probs, want.numpy(), rtol=1e-13, atol=0)


def test_reference_tie_order_and_nonfinite_rows():
    logits = np.array([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, np.nan, 1.0, 2.0], [np.inf, 0.0, 0.0, 0.0]], dtype=np.float32)
    probs, idx, top = eval_ref.classify(logits, 3)
    assert idx.tolist() == [[1, 2, 0], [0, 1, 2], [-1, -1, -1], [-1, -1, -1]]
    assert np.isnan(probs[2:]).all() and np.isnan(top[2:]).all() and np.isfinite(probs[:2]).all()
    st = eval_ref.eval_accumulate(eval_ref.empty_state(4, 4), logits, [2, -100, 1, 7], 4)
    assert (st["n"], st["n_ignored"], st["n_nonfinite"], st["bad_label"]) == (1, 1, 1, True)
    assert st["confusion"][2, 1] == 1 and st["topk_correct"].tolist() == [0, 1, 1, 1, 1, 1, 1, 1]


def test_reference_temperature_fit_finds_the_scale():
    rng = np.random.default_rng(2)
    base = rng.normal(size=(4097, 31)) * 2
    p = eval_ref.softmax(base)
    labels = np.array([rng.choice(31, p=row) for row in p])
    for scale in (4.0, 0.25, 1.0):
        logits = (base * scale).astype(np.float32)
        beta, f1, fb = eval_ref.temperature_fit(logits, labels, 20)
        assert beta == pytest.approx(1.0 / scale, rel=0.05)            # the sample's optimum, near the generating 1 / scale
        assert fb <= f1 and f1 == pytest.approx(eval_ref.nll(logits, labels, 1.0), rel=1e-12)
        assert fb == pytest.approx(eval_ref.nll(logits, labels, beta), rel=1e-12)
        b32 = eval_ref.temperature_fit(logits, labels, 20, dtype=np.float32)[0]
        assert b32 == pytest.approx(beta, rel=1e-4)
    sep = rng.normal(size=(64, 5)).astype(np.float32)
    assert eval_ref.temperature_fit(sep, sep.argmax(1), 20)[0] == 64.0   # separable: f' < 0 everywhere, clamped


def _hand_state():
    """4 bins, 10 rows: bin 1 holds 4 rows (3 correct, confidences sum 1.6), bin 3 holds 6 (3 correct, sum 5.4)."""
    st = eval_ref.empty_state(2, 4)
    st["confusion"][:] = [[4, 1], [3, 2]]
    st["n"] = 10
    st["topk_correct"][:] = [6, 10, 10, 10, 10, 10, 10, 10]
    st["nll_sum"] = 5.0
    st["bin_count"][:] = [0, 4, 0, 6]
    st["bin_correct"][:] = [0, 3, 0, 3]
    st["bin_conf_sum"][:] = [0.0, 1.6, 0.0, 5.4]
    return st


def test_report_from_hand_built_state():
    rep = metrics.report_from_state(_hand_state(), target_names=["no", "yes"])
    assert rep["accuracy"] == pytest.approx(0.6) and rep["top1"] == pytest.approx(0.6) and rep["top3"] == 1.0 and rep["top5"] == 1.0
    assert rep["nll"] == pytest.approx(0.5)
    # |0.75 - 0.4| = 0.35 on 4 rows, |0.5 - 0.9| = 0.4 on 6 rows
    assert rep["ece"] == pytest.approx((4 * 0.35 + 6 * 0.4) / 10, rel=1e-12)
    assert rep["mce"] == pytest.approx(0.4, rel=1e-12)
    rel = rep["reliability"]
    assert rel["count"].tolist() == [0, 4, 0, 6] and np.isnan(rel["accuracy"][[0, 2]]).all()
    assert rel["lo"].tolist() == [0.0, 0.25, 0.5, 0.75] and rel["hi"][-1] == 1.0
    cls = rep["classification"]
    assert cls["no"]["precision"] == pytest.approx(4 / 7) and cls["no"]["recall"] == pytest.approx(0.8) and cls["yes"]["support"] == 5
    assert cls["accuracy"] == pytest.approx(0.6) and cls["macro avg"]["support"] == 10
    import json
    json.dumps(metrics.calibration_json(rep))
    bad = _hand_state()
    bad["n"] = 11
    with pytest.raises(ValueError):
        metrics.report_from_state(bad)


def test_merge_is_additive_and_unpack_round_trips():
    rng = np.random.default_rng(9)
    logits = rng.normal(size=(120, 5)).astype(np.float32)
    labels = rng.integers(0, 5, size=120)
    labels[::17] = -100
    whole = eval_ref.eval_accumulate(eval_ref.empty_state(5, 8), logits, labels, 8)
    a = eval_ref.eval_accumulate(eval_ref.empty_state(5, 8), logits[:50], labels[:50], 8)
    b = eval_ref.eval_accumulate(eval_ref.empty_state(5, 8), logits[50:], labels[50:], 8)
    m = metrics.merge(a, b)
    for k in ("confusion", "topk_correct", "bin_count", "bin_correct"):
        assert np.array_equal(m[k], whole[k]), k
    assert (m["n"], m["n_ignored"], m["n_nonfinite"]) == (whole["n"], whole["n_ignored"], 0)
    assert m["nll_sum"] == pytest.approx(whole["nll_sum"], rel=1e-13) and np.allclose(m["bin_conf_sum"], whole["bin_conf_sum"], rtol=1e-13)
    with pytest.raises(ValueError):
        metrics.merge(a, eval_ref.empty_state(5, 9))
    # the packed device layout: words in header order
    words = np.concatenate([whole["confusion"].ravel(), [whole["n"]], whole["topk_correct"],
                            np.array([whole["nll_sum"]]).view(np.int64), whole["bin_count"], whole["bin_correct"],
                            whole["bin_conf_sum"].view(np.int64), [whole["n_ignored"], whole["n_nonfinite"]]]).astype(np.int64)
    assert len(words) == metrics.field_words(5, 8)
    words = np.concatenate([words, np.full(metrics.state_words(5, 8) - len(words), 123, dtype=np.int64)])      # the kernels' scratch area
    back = metrics.unpack_state(words, 5, 8)
    assert np.array_equal(back["confusion"], whole["confusion"]) and back["nll_sum"] == whole["nll_sum"]
    assert np.array_equal(back["bin_conf_sum"], whole["bin_conf_sum"]) and back["n_ignored"] == whole["n_ignored"]


def test_argument_validation_without_a_gpu():
    lib = _native.lib()
    assert lib.sir_eval_state_bytes(31, 15) == 8 * metrics.state_words(31, 15) == 8 * (31 * 31 + 12 + 45 + 64 * 16)
    for c, m in ((0, 15), (65, 15), (31, 0), (31, 65)):
        assert lib.sir_eval_state_bytes(c, m) == 0
        with pytest.raises(ValueError):
            metrics.EvalAccumulator(c, m)
    assert lib.sir_temperature_fit_workspace_bytes(0) == 0 and lib.sir_temperature_fit_workspace_bytes((1 << 22) + 1) == 0
    assert lib.sir_temperature_fit_workspace_bytes(1) >= 64 + 32
    assert lib.sir_temperature_fit_workspace_bytes(1 << 22) >= lib.sir_temperature_fit_workspace_bytes(4097)
    with pytest.raises(ValueError):
        metrics.EvalAccumulator(31, inv_temperature=0.0)
    with pytest.raises(ValueError):
        metrics.EvalAccumulator(31, inv_temperature=float("nan"))
    # the C entry points refuse bad arguments before touching a device (no launch: this runs without a GPU)
    one = (np.zeros(64, dtype=np.float32)).ctypes.data
    assert lib.sir_classify(None, one, 1, 2, None, 1, None, one, one, None) == _native.SIR_EINVAL
    assert lib.sir_eval_accumulate(None, one, one, 1, 2, None, 15, one, 1 << 20, None) == _native.SIR_EINVAL
    assert lib.sir_temperature_fit(None, one, one, 1, 2, 20, one, one, 1 << 20, None) == _native.SIR_EINVAL
    from sir_amd.scripts import classify_results
    with pytest.raises(ValueError):
        classify_results.inv_temperature_of(0)
    classify_results.check_route(False, None, None)
    classify_results.check_route(True, 2.0, 0.5)
    for kw in ((2.0, None), (None, 0.5)):
        with pytest.raises(ValueError):
            classify_results.check_route(False, *kw)
    assert classify_results.inv_temperature_of(None) is None and classify_results.inv_temperature_of(4) == 0.25
    if not torch.cuda.is_available():
        from sir_amd import ops
        with pytest.raises(_native.SirError):
            ops.classify(torch.zeros(2, 3))
        with pytest.raises(_native.SirError):
            metrics.EvalAccumulator(3).update(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))
        with pytest.raises(_native.SirError):
            metrics.fit_temperature(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))
