"""GPU: sir_classify, sir_eval_accumulate and sir_temperature_fit against the float64 reference (tests/eval_ref.py), their
tie / non-finite / label rules, stream capture, and the Python surface on top (ops.classify, CNNAudioGRU.classify,
EvalAccumulator, fit_temperature, results_from_logits, evaluate(device_metrics))."""
import json
import os
import types

import numpy as np
import pytest
import torch

import eval_ref
from sir_amd import _native, metrics, ops, synth

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (1, 1), (63, 31), (65, 31), (257, 64), (1041, 31)]
BETAS = [None, 0.5, 3.0]
PROB_TOL = 64 * 2.0 ** -24          # one rounding per class in the denominator plus the exponentials' few ulp


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).cuda()


def _spread_logits(b, c, seed):
    """Rows whose values are a shuffled, jittered grid times a per-row scale: every pair of logits of a row differs by more
    than 1e-4 in float64 (asserted), so no ranking or probability depends on a rounding."""
    rng = np.random.default_rng(seed)
    grid = np.stack([rng.permutation(c) for _ in range(b)]).astype(np.float64)
    x = (grid * 0.37 + rng.uniform(0.0, 0.1, size=(b, c))) * rng.uniform(0.05, 1.0, size=(b, 1)) - rng.uniform(0, 4, size=(b, 1))
    x = x.astype(np.float32)
    if c > 1:
        gaps = np.diff(np.sort(x.astype(np.float64), axis=1), axis=1)
        assert gaps.min() > 1e-4
    return x


_logit_cache = {}


def _logits(b, c):
    if (b, c) not in _logit_cache:
        _logit_cache[(b, c)] = _spread_logits(b, c, seed=1000 * b + c)
    return _logit_cache[(b, c)]


# ---- sir_classify ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b,c", SHAPES)
def test_classify_matches_reference(b, c):
    x = _logits(b, c)
    xd = _dev(x)
    for k in sorted({1, min(3, c), min(8, c)}):
        for beta in BETAS:
            want_p, want_i, want_t = eval_ref.classify(x, k, beta)
            idx, top, probs = ops.classify(xd, k=k, inv_temperature=beta, want_probs=True)
            assert idx.dtype == torch.int32 and idx.shape == (b, k) and top.shape == (b, k)
            assert np.array_equal(idx.cpu().numpy(), want_i), (k, beta)
            err_t = np.abs(top.cpu().numpy().astype(np.float64) - want_t).max()
            err_p = np.abs(probs.cpu().numpy().astype(np.float64) - want_p).max()
            print(f"classify B={b} C={c} k={k} beta={beta}: top-k prob err {err_t:.2e}, softmax err {err_p:.2e} (bound {PROB_TOL:.2e})")
            assert err_t <= PROB_TOL and err_p <= PROB_TOL
    # a device scalar as inv_temperature, and no probs buffer
    idx2, top2 = ops.classify(xd, k=1, inv_temperature=torch.tensor([3.0, 7.0, 7.0], device="cuda"))
    assert torch.equal(idx2, idx[:, :1]) and torch.equal(top2, top[:, :1])


def test_classify_tie_order():
    c, k = 31, 3
    x = np.tile(np.linspace(-3.0, -1.0, c, dtype=np.float32), (5, 1))
    x[0, [7, 20]] = 5.0                                     # two equal maxima
    x[1, 5], x[1, 9], x[1, [2, 11, 30]] = 10.0, 9.0, 8.0    # three equal, the tie straddles position k: ranks 2, 3, 4
    x[2, :] = 0.25                                          # all C equal
    x[3, [30, 0]] = 1.0                                     # first and last lane
    x[4, 4], x[4, 3] = 0.0, -0.0                            # +0 and -0 compare equal: the lower index first
    x[4, 5:] = -1.0
    x[4, :3] = -2.0
    for beta in BETAS:
        idx, top = ops.classify(_dev(x), k=k, inv_temperature=beta)
        got = idx.cpu().numpy()
        assert np.array_equal(got, eval_ref.classify(x, k, beta)[1])
        assert got[0].tolist() == [7, 20, 30] and got[1].tolist() == [5, 9, 2] and got[2].tolist() == [0, 1, 2]
        assert got[3].tolist() == [0, 30, 29] and got[4].tolist()[:2] == [3, 4]
        t = top.cpu().numpy()
        assert t[2, 0] == t[2, 1] == t[2, 2] and abs(t[2, 0] - 1.0 / c) < 1e-7
    idx8, _ = ops.classify(_dev(x[2:3, :8].copy()), k=8)
    assert idx8.cpu().numpy().tolist() == [list(range(8))]


def test_classify_nonfinite_rows_leave_neighbours_alone():
    x = _logits(65, 31).copy()
    clean = ops.classify(_dev(x), k=3, want_probs=True)
    x[3, 30] = np.nan
    x[40, 0] = np.inf
    x[64, 17] = -np.inf
    idx, top, probs = ops.classify(_dev(x), k=3, want_probs=True)
    bad = [3, 40, 64]
    good = [i for i in range(65) if i not in bad]
    assert (idx[bad] == -1).all() and torch.isnan(top[bad]).all() and torch.isnan(probs[bad]).all()
    for got, want in zip((idx, top, probs), clean):
        assert torch.equal(got[good], want[good])


def test_classify_argument_validation():
    x = _dev(_logits(63, 31))
    for k in (0, 9, -1):
        with pytest.raises(_native.SirError):
            ops.classify(x, k=k)
    with pytest.raises(_native.SirError):
        ops.classify(x[:, :2].contiguous(), k=3)                     # k > C
    with pytest.raises(_native.SirError):
        ops.classify(torch.zeros(4, 65, device="cuda"), k=1)
    with pytest.raises(_native.SirError):
        ops.classify(x, inv_temperature=-1.0)
    lib, h = _native.lib(), ops.get_featurizer().handle
    out_i = torch.full((63, 3), 77, dtype=torch.int32, device="cuda")
    out_p = torch.zeros((63, 3), device="cuda")
    assert lib.sir_classify(h, x.data_ptr(), 63, 31, None, 9, None, out_i.data_ptr(), out_p.data_ptr(), None) == _native.SIR_EINVAL
    assert lib.sir_classify(h, x.data_ptr(), 63, 65, None, 3, None, out_i.data_ptr(), out_p.data_ptr(), None) == _native.SIR_EINVAL
    assert lib.sir_classify(h, x.data_ptr(), 63, 31, None, 3, None, None, out_p.data_ptr(), None) == _native.SIR_EINVAL
    assert lib.sir_classify(h, x.data_ptr(), (1 << 30) + 1, 31, None, 3, None, out_i.data_ptr(), out_p.data_ptr(), None) == _native.SIR_EINVAL
    torch.cuda.synchronize()
    assert (out_i == 77).all()                                       # a refused call writes nothing
    idx_np, _ = ops.classify(x, k=np.int64(3))                       # numpy integers are integers
    assert torch.equal(idx_np, ops.classify(x, k=3)[0])
    with pytest.raises(_native.SirError):
        ops.classify(x, k=3.0)


def test_top1_is_the_models_argmax_padded_and_ragged():
    from sir_amd.models.models import CNNAudioGRU
    model = CNNAudioGRU(31)
    model.load_state_dict(synth.synth_state_dict(31, seed=0))
    model = model.cuda().eval()
    g = torch.Generator().manual_seed(5)
    feats = (torch.randn(65, 64, 24, generator=g) * 20 - 30).cuda()
    logits_p, amax = model.predict(feats)
    logits, idx, prob = model.classify(feats, k=3)
    assert torch.equal(logits, logits_p) and torch.equal(idx[:, 0].to(torch.int64), amax)
    for beta in (0.5, 3.0):
        assert torch.equal(model.classify(feats, k=1, inv_temperature=beta)[1][:, 0].to(torch.int64), amax)
    lengths = [8 + (7 * i) % 17 for i in range(65)]
    logits_r, amax_r = model.predict(feats, lengths=lengths)
    logits_c, idx_r, prob_r = model.classify(feats, lengths=lengths, k=3)
    assert torch.equal(logits_c, logits_r) and torch.equal(idx_r[:, 0].to(torch.int64), amax_r)
    want = eval_ref.classify(logits_r.cpu().numpy(), 3)
    assert np.array_equal(idx_r.cpu().numpy(), want[1])
    assert np.abs(prob_r.cpu().numpy() - want[2]).max() <= PROB_TOL
    ops.check_status()


# ---- sir_eval_accumulate -----------------------------------------------------------------------------------------------------

def _eval_batch(b, c, n_bins, beta, seed):
    """logits [b, c] and labels (about half of them the prediction) whose float64 confidence lies at least 1e-4 from every
    bin edge (asserted): the bin of a row cannot depend on an fp32 rounding."""
    def clear_of_edges(rows):
        # distance of the confidence to the nearest edge between two bins (j / n_bins, 0 < j < n_bins; 1.0 is no such edge)
        pos = eval_ref.confidences(rows, beta) * n_bins
        near = np.round(pos)
        return ~((near > 0) & (near < n_bins) & (np.abs(pos - near) < 1e-4 * n_bins))

    x = _spread_logits(2 * b + 8, c, seed)
    x = x[clear_of_edges(x)][:b]
    assert x.shape[0] == b and clear_of_edges(x).all()
    rng = np.random.default_rng(seed + 1)
    labels = np.where(rng.random(b) < 0.5, x.argmax(1), rng.integers(0, c, size=b)).astype(np.int64)
    return x, labels


def _assert_state(got, want, what=""):
    for k in ("confusion", "topk_correct", "bin_count", "bin_correct"):
        assert np.array_equal(got[k], want[k]), (what, k)
    for k in ("n", "n_ignored", "n_nonfinite"):
        assert got[k] == want[k], (what, k)
    rel_nll = abs(got["nll_sum"] - want["nll_sum"]) / max(abs(want["nll_sum"]), 1e-300)
    occ = want["bin_count"] > 0
    rel_conf = (np.abs(got["bin_conf_sum"] - want["bin_conf_sum"])[occ] / want["bin_conf_sum"][occ]).max() if occ.any() else 0.0
    print(f"eval state {what}: nll_sum rel err {rel_nll:.2e}, bin_conf_sum rel err {rel_conf:.2e} (bound 1e-6)")
    assert rel_nll <= 1e-6 and rel_conf <= 1e-6
    assert (got["bin_conf_sum"][~occ] == 0).all()


@pytest.mark.parametrize("c,n_bins,beta", [(31, 15, None), (31, 64, 0.5), (64, 1, 3.0), (2, 15, None), (1, 15, None), (32, 15, None),
                                           (33, 15, None)])
def test_eval_accumulate_three_updates_match_one_reference_pass(c, n_bins, beta):
    parts = [_eval_batch(b, c, n_bins, beta, seed=31 * b + c) for b in (63, 1, 257)]
    acc = metrics.EvalAccumulator(c, n_bins=n_bins, inv_temperature=beta)
    for x, y in parts:
        acc.update(_dev(x), _dev(y))
    got = acc.state_arrays()
    x_all, y_all = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    want = eval_ref.eval_accumulate(eval_ref.empty_state(c, n_bins), x_all, y_all, n_bins, beta)
    _assert_state(got, want, f"C={c} bins={n_bins} beta={beta}")
    assert got["n"] == 321
    rep = acc.result()
    assert rep["accuracy"] == pytest.approx(np.trace(want["confusion"]) / 321, rel=1e-15)
    # a second run of the same updates: bit-identical state, doubles included
    again = metrics.EvalAccumulator(c, n_bins=n_bins, inv_temperature=beta)
    for x, y in parts:
        again.update(_dev(x), _dev(y))
    assert torch.equal(again._state, acc._state)
    acc.reset()
    assert acc.state_arrays()["n"] == 0 and (acc._state == 0).all()
    ops.check_status()


def test_eval_accumulate_ignored_bad_and_nonfinite_rows():
    c, n_bins = 31, 15
    x, y = _eval_batch(65, c, n_bins, None, seed=77)
    y[[1, 9, 33]] = -100
    x[9, 3] = np.nan                       # ignored wins over non-finite
    x[[20, 64], 5] = [np.inf, np.nan]
    y[50] = c                              # out of range: left out, status raised
    x[50, 0] = np.nan                      # ... whatever its logits hold
    ops.check_status()
    acc = metrics.EvalAccumulator(c, n_bins=n_bins)
    acc.update(_dev(x), _dev(y))
    got = acc.state_arrays()
    want = eval_ref.eval_accumulate(eval_ref.empty_state(c, n_bins), x, y, n_bins)
    assert want["bad_label"] and (want["n"], want["n_ignored"], want["n_nonfinite"]) == (65 - 6, 3, 2)
    _assert_state(got, want, "mixed rows")
    with pytest.raises(_native.SirError, match="label outside"):
        ops.check_status()
    ops.check_status()                     # raised once, then clear
    y[50] = -1
    acc.update(_dev(x), _dev(y))
    with pytest.raises(_native.SirError):
        ops.check_status()
    _assert_state(acc.state_arrays(), metrics.merge(want, want), "mixed rows twice")


def test_eval_accumulate_refuses_bad_arguments():
    lib, h = _native.lib(), ops.get_featurizer().handle
    x, y = _dev(_logits(63, 31)), torch.zeros(63, dtype=torch.int64, device="cuda")
    need = lib.sir_eval_state_bytes(31, 15)
    state = torch.zeros(need // 8, dtype=torch.int64, device="cuda")
    call = lambda c, m, nbytes: lib.sir_eval_accumulate(h, x.data_ptr(), y.data_ptr(), 63, c, None, m, state.data_ptr(), nbytes, None)
    assert call(31, 15, need - 8) == -2                               # SIR_ENOMEM
    assert call(31, 0, need) == _native.SIR_EINVAL and call(31, 65, 1 << 20) == _native.SIR_EINVAL
    assert call(65, 15, 1 << 20) == _native.SIR_EINVAL
    assert lib.sir_eval_accumulate(h, x.data_ptr(), y.data_ptr(), (1 << 30) + 1, 31, None, 15, state.data_ptr(), need, None) == _native.SIR_EINVAL
    assert lib.sir_eval_accumulate(h, x.data_ptr(), y.data_ptr(), 63, 31, None, 15, state.data_ptr() + 4, need, None) == _native.SIR_EINVAL
    torch.cuda.synchronize()
    assert (state == 0).all()
    assert call(31, 15, need) == 0
    assert int(state[31 * 31]) == 63
    with pytest.raises(_native.SirError):
        metrics.EvalAccumulator(31).update(x, y.to(torch.int32))
    with pytest.raises(_native.SirError):
        metrics.EvalAccumulator(30).update(x, y)


# ---- sir_temperature_fit -----------------------------------------------------------------------------------------------------

def _fit_case(kind, n, c=31):
    rng = np.random.default_rng({"over": 1, "under": 2, "separable": 3, "optimal": 4}[kind] * 10000 + n)
    base = rng.normal(size=(n, c)) * 1.5
    if kind == "separable":
        x = base.astype(np.float32)
        return x, x.argmax(1).astype(np.int64)
    p = eval_ref.softmax(base)
    cdf = np.cumsum(p, axis=1)
    labels = np.minimum((rng.random((n, 1)) > cdf).sum(1), c - 1).astype(np.int64)       # drawn from the softmax at scale 1
    scale = {"over": 4.0, "under": 0.25, "optimal": 1.0}[kind]
    return (base * scale).astype(np.float32), labels


@pytest.mark.parametrize("n", [64, 4097])
@pytest.mark.parametrize("kind", ["over", "under", "separable", "optimal"])
def test_temperature_fit_matches_the_newton_reference(kind, n):
    x, y = _fit_case(kind, n)
    b64, f1_64, _ = eval_ref.temperature_fit(x, y, 20)
    b32 = eval_ref.temperature_fit(x, y, 20, dtype=np.float32)[0]
    out = metrics.fit_temperature(_dev(x), _dev(y), iters=20)
    assert out.shape == (3,) and out.dtype == torch.float32 and out.is_cuda
    beta, nll1, nllb = (float(v) for v in out.cpu())
    ref_err = abs(b32 - b64)
    tol = max(4.0 * ref_err, 1e-6 * b64)
    err = abs(beta - b64)
    print(f"temperature fit {kind} N={n}: beta f64 {b64:.9g} f32-numpy {b32:.9g} gpu {beta:.9g}; |gpu - f64| = {err:.3e}, "
          f"|f32 - f64| = {ref_err:.3e}, ratio {err / ref_err if ref_err else float('nan'):.3g}, tolerance {tol:.3e}")
    assert err <= tol
    if kind == "separable":
        assert b64 == 64.0 and beta == 64.0
    elif kind != "optimal":
        assert beta == pytest.approx(0.25 if kind == "over" else 4.0, rel=0.5 if n == 64 else 0.1)
    f_gpu = eval_ref.nll(x, y, np.float64(np.float32(beta)))
    assert f_gpu <= eval_ref.nll(x, y, 1.0)
    assert nll1 == pytest.approx(f1_64, rel=1e-6) and nllb == pytest.approx(f_gpu, rel=1e-6)
    # the result is a valid inv_temperature as it stands: the calibrated NLL of an accumulator is the fitted one
    acc = metrics.EvalAccumulator(31, inv_temperature=out).update(_dev(x), _dev(y))
    assert acc.result()["nll"] == pytest.approx(f_gpu, rel=2e-6)
    again = metrics.fit_temperature(_dev(x), _dev(y), iters=20)
    assert torch.equal(again, out)                                    # ordered sums: run-to-run identical


def test_temperature_fit_rows_and_arguments():
    x, y = _fit_case("over", 257)
    y2, x2 = y.copy(), x.copy()
    y2[[0, 100]] = -100
    x2[7, 2] = np.inf
    keep = np.ones(257, dtype=bool)
    keep[[0, 100, 7]] = False
    want = eval_ref.temperature_fit(x[keep], y[keep], 20)
    assert eval_ref.temperature_fit(x2, y2, 20) == want
    got = metrics.fit_temperature(_dev(x2), _dev(y2)).cpu()
    assert float(got[0]) == pytest.approx(want[0], rel=1e-5) and float(got[2]) == pytest.approx(want[2], rel=1e-5)
    ops.check_status()
    zero = metrics.fit_temperature(_dev(x), _dev(y), iters=0).cpu()
    assert float(zero[0]) == 1.0 and float(zero[1]) == float(zero[2]) == pytest.approx(eval_ref.nll(x, y, 1.0), rel=1e-6)
    y2[5] = 31
    metrics.fit_temperature(_dev(x2), _dev(y2))
    with pytest.raises(_native.SirError, match="label outside"):
        ops.check_status()
    ops.check_status()
    lib, h = _native.lib(), ops.get_featurizer().handle
    xd, yd = _dev(x), _dev(y)
    need = lib.sir_temperature_fit_workspace_bytes(257)
    ws = torch.zeros(need // 8 + 1, dtype=torch.int64, device="cuda")
    out = torch.full((3,), -7.0, device="cuda")
    assert lib.sir_temperature_fit(h, xd.data_ptr(), yd.data_ptr(), 257, 31, 20, out.data_ptr(), ws.data_ptr(), need - 8, None) == -2
    assert lib.sir_temperature_fit(h, xd.data_ptr(), yd.data_ptr(), 257, 31, -1, out.data_ptr(), ws.data_ptr(), need, None) == _native.SIR_EINVAL
    assert lib.sir_temperature_fit(h, xd.data_ptr(), yd.data_ptr(), 257, 65, 20, out.data_ptr(), ws.data_ptr(), need, None) == _native.SIR_EINVAL
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    with pytest.raises(_native.SirError):
        metrics.fit_temperature(xd, yd, iters=1001)


# ---- stream capture ------------------------------------------------------------------------------------------------------------

def test_classify_and_accumulate_under_graph_capture():
    c, n_bins = 31, 15
    x, y = _eval_batch(257, c, n_bins, None, seed=9)
    xd, yd = _dev(x), _dev(y)
    acc = metrics.EvalAccumulator(c, n_bins=n_bins)
    acc.update(xd, yd)                                   # allocates the state outside the capture
    idx_eager, top_eager = ops.classify(xd, k=3)
    single = acc.state_arrays()
    acc.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        idx, top = ops.classify(xd, k=3)
        acc.update(xd, yd)
    assert acc.state_arrays()["n"] == 0                  # capturing runs nothing
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    twice = acc.state_arrays()
    for k in ("confusion", "topk_correct", "bin_count", "bin_correct"):
        assert np.array_equal(twice[k], 2 * single[k]), k
    assert (twice["n"], twice["n_ignored"], twice["n_nonfinite"]) == (2 * 257, 0, 0)
    assert twice["nll_sum"] == pytest.approx(2 * single["nll_sum"], rel=1e-12)
    assert torch.equal(idx, idx_eager) and torch.equal(top, top_eager)
    ops.check_status()


# ---- Python surface ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """The synthetic split of tests/test_pipeline_gpu.py (24 clips, 4 labels, two unreadable files) with its feature cache, a
    label map and a checkpoint of synthetic weights."""
    import pandas as pd
    from test_pipeline_gpu import LABELS, _make_corpus
    from sir_amd.scripts import precompute_features as pf
    root = tmp_path_factory.mktemp("eval_corpus")
    rows = _make_corpus(str(root / "wav"))
    csv = root / "all_data.csv"
    pd.DataFrame(rows).to_csv(csv, index=False)
    lm = root / "label_map.json"
    lm.write_text(json.dumps({l: i for i, l in enumerate(sorted(LABELS))}))
    cache_dir = str(root / "cache")
    pf.precompute_dataset_features(str(csv), cache_dir)
    ckpt = root / "ckpt" / "best_model.pt"
    os.makedirs(ckpt.parent)
    sd = synth.synth_state_dict(31, seed=3)
    sd["fc.bias"] = sd["fc.bias"].clone()
    sd["fc.bias"][:4] += 50.0         # predictions inside the label map's four classes: some are right (see the test below)
    torch.save(sd, ckpt)
    return types.SimpleNamespace(root=root, rows=rows, csv=str(csv), label_map=str(lm), cache_dir=cache_dir, ckpt=str(ckpt))


def test_evaluate_device_metrics_writes_the_same_report(corpus):
    from sir_amd.scripts import evaluate as ev
    args = types.SimpleNamespace(test_csv=corpus.csv, label_map=corpus.label_map, model_path=corpus.ckpt)
    base = {"batch_size": 8, "num_workers": 0, "cache_dir": corpus.cache_dir, "use_feature_cache": True}
    host_cfg = dict(base, save_path=str(corpus.root / "host"))
    dev_cfg = dict(base, save_path=str(corpus.root / "dev"), device_metrics=True)
    acc_host = ev.evaluate(args, host_cfg)
    acc_dev = ev.evaluate(args, dev_cfg)
    # (with not one correct prediction sklearn prints the supports as floats, "6.0": its true-positive histogram is then a
    # float array.  metrics.format_report always prints integers, so the comparison needs a model that is right sometimes.)
    assert acc_dev == acc_host and acc_host > 0
    read = lambda cfg, name: open(os.path.join(cfg["save_path"], "evaluation_results", name)).read()
    assert read(dev_cfg, "classification_report.txt") == read(host_cfg, "classification_report.txt")
    assert not os.path.exists(os.path.join(host_cfg["save_path"], "evaluation_results", "calibration.json"))
    for cfg in (host_cfg, dev_cfg):                      # both routes plot the matrix
        assert os.path.getsize(os.path.join(cfg["save_path"], "evaluation_results", "confusion_matrix.png")) > 0
    calib = json.loads(read(dev_cfg, "calibration.json"))
    assert calib["n"] == 24 and calib["accuracy"] == acc_host and calib["inv_temperature"] == 1.0
    assert sum(calib["reliability"]["count"]) == 24 and len(calib["reliability"]["count"]) == 15
    assert 0.0 <= calib["ece"] <= calib["mce"] <= 1.0 and calib["top1"] <= calib["top3"] <= calib["top5"]
    # --fit_temperature writes temperature.json beside the checkpoint; --temperature_file reads it back
    fit_args = types.SimpleNamespace(**vars(args), fit_temperature=corpus.csv)
    assert ev.evaluate(fit_args, dict(dev_cfg, save_path=str(corpus.root / "fit"))) == acc_host
    tpath = os.path.join(os.path.dirname(corpus.ckpt), "temperature.json")
    info = json.load(open(tpath))
    assert info["n"] == 24 and 1.0 / 64 <= info["inv_temperature"] <= 64 and info["nll_after"] <= info["nll_before"] + 1e-6
    fit_calib = json.loads(read({"save_path": str(corpus.root / "fit")}, "calibration.json"))
    assert fit_calib["inv_temperature"] == info["inv_temperature"] and fit_calib["nll"] == pytest.approx(info["nll_after"], rel=1e-5)
    file_args = types.SimpleNamespace(**vars(args), temperature_file=tpath)
    assert ev.evaluate(file_args, dict(dev_cfg, save_path=str(corpus.root / "file"))) == acc_host
    assert json.loads(read({"save_path": str(corpus.root / "file")}, "calibration.json"))["nll"] == fit_calib["nll"]


def _same_results(a, b, tol=4e-6):
    assert set(b) >= set(a) and b["predicted_label"] == a["predicted_label"]
    assert abs(b["confidence"] - a["confidence"]) <= tol
    assert [p["label"] for p in b["top_predictions"]] == [p["label"] for p in a["top_predictions"]]
    assert all(abs(p["probability"] - q["probability"]) <= tol for p, q in zip(b["top_predictions"], a["top_predictions"]))


def test_predict_many_on_device_matches_the_host_route(corpus):
    """predict_frontend.predict_many(on_device=True) against its own default route and against test_model.predict_many (the
    same features and forward at the default front-end): same files fail, same labels, confidences within 4e-6."""
    from sir_amd.models.models import CNNAudioGRU
    from sir_amd.scripts import predict_frontend, test_model
    model = CNNAudioGRU(31)
    model.load_state_dict(torch.load(corpus.ckpt))
    model = model.cuda().eval()
    label_map = {f"intent_{i:02d}": i for i in range(31)}
    paths = [r["path"] for r in corpus.rows]
    dev = torch.device("cuda")
    host = predict_frontend.predict_many(model, paths, label_map, dev)
    legacy = test_model.predict_many(model, paths, label_map, dev)
    ondev = predict_frontend.predict_many(model, paths, label_map, dev, on_device=True)
    failed = [r is None for r in host]
    assert failed == [r is None for r in ondev] == [r is None for r in legacy] and sum(failed) == 2
    assert len({round(r["confidence"], 5) for r in ondev if r}) > 1     # files differ: a wrong keep -> file mapping would show below
    for a, b, c in zip(host, ondev, legacy):
        if a is not None:
            assert set(b) == set(a)
            _same_results(a, b)
            _same_results(c, b)
    none = predict_frontend.predict_many(model, paths, label_map, dev, on_device=True, min_confidence=0)
    every = predict_frontend.predict_many(model, paths, label_map, dev, on_device=True, min_confidence=1.1)
    assert [r is None for r in none] == failed == [r is None for r in every]
    assert all(not r["rejected"] for r in none if r) and all(r["rejected"] for r in every if r)
    for a, b in zip(ondev, none):
        if a is not None:
            _same_results(a, b, tol=0.0)
    cool = predict_frontend.predict_many(model, paths, label_map, dev, on_device=True, temperature=4.0, min_confidence=0.5)
    for a, b in zip(ondev, cool):
        if a is not None:
            assert b["predicted_label"] == a["predicted_label"] and b["confidence"] <= a["confidence"] + 1e-7
            assert b["rejected"] == (not b["confidence"] >= 0.5)
    # temperature is really 1 / beta: the on-device confidences at T = 4 are the reference softmax of logits / 4
    feats = test_model._get_extractor().extract_batch([p for p, f in zip(paths, failed) if not f], max_duration=600.0)
    batch = torch.stack([test_model._pad_or_trim(f.unsqueeze(0), test_model.MAX_LENGTH)[0] for f in feats]).cuda()
    with torch.no_grad():
        logits = model(batch).cpu().numpy()
    conf = eval_ref.confidences(logits, 0.25)
    got = np.array([r["confidence"] for r in cool if r])
    assert np.abs(got - conf).max() <= 4e-6
    # the arguments of the device route are refused without it, not dropped
    for kw in ({"temperature": 2.0}, {"min_confidence": 0.5}):
        with pytest.raises(ValueError):
            predict_frontend.predict_many(model, paths, label_map, dev, **kw)
    with pytest.raises(_native.SirError):
        from sir_amd.scripts import classify_results
        classify_results.results_from_logits(torch.zeros(2, 31, device="cuda"), {}, k=9)


def test_pipeline_slot_closes_when_then_raises():
    from sir_amd.models.models import CNNAudioGRU
    from sir_amd.pipeline import BatchPipeline
    model = CNNAudioGRU(31)
    model.load_state_dict(synth.synth_state_dict(31, seed=0))
    model = model.cuda().eval()
    pipe = BatchPipeline(model, n_streams=2)
    feats = (torch.randn(4, 64, 24, generator=torch.Generator().manual_seed(3)) * 20 - 30).cuda()

    def boom(slot, out):
        raise RuntimeError("then failed")

    for i in range(3):                                  # a slot left open would make the third begin fail (two slots)
        with pytest.raises(RuntimeError, match="then failed"):
            pipe.infer(i, feats, then=boom)
    seen = []
    pipe.infer(3, feats, then=lambda slot, out: seen.append(slot))
    pipe.synchronize()
    assert len(seen) == 1
    ops.check_status()


def test_recognize_recordings_on_device_matches_the_host_route():
    from sir_amd.models.models import CNNAudioGRU
    from sir_amd.scripts.testing import IntentRecognizer
    utt = synth.synth_clips(3, 40000, seed=78).numpy()
    z = lambda chunks: np.zeros(chunks * 1024, dtype=np.float32)
    recs = [np.concatenate([z(8), utt[0, :24 * 1024], z(24), utt[1, :32 * 1024], z(20)]), np.concatenate([utt[2, :16 * 1024], z(32)])]
    torch.manual_seed(6)
    model = CNNAudioGRU(5).cuda().eval()
    reco = IntentRecognizer.from_model(model, {f"intent_{i}": i for i in range(5)}, torch.device("cuda"))
    for pad_to in (200, None):
        host = reco.recognize_recordings(recs, pad_to=pad_to)
        ondev = reco.recognize_recordings(recs, pad_to=pad_to, on_device=True, min_confidence=1.1)
        assert [len(f) for f in host] == [len(f) for f in ondev] == [2, 1]
        for a, b in zip([u for f in host for u in f], [u for f in ondev for u in f]):
            assert (b["start"], b["end"], b["predicted_label"]) == (a["start"], a["end"], a["predicted_label"])
            assert abs(b["confidence"] - a["confidence"]) <= 4e-6 and b["rejected"] and "rejected" not in a
            assert [p["label"] for p in b["top_predictions"]] == [p["label"] for p in a["top_predictions"]]
    with pytest.raises(ValueError):
        reco.recognize_recordings(recs, min_confidence=0.5)
